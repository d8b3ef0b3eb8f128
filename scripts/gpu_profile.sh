#!/bin/bash
# Round profile: rocprofv3 kernel-trace stats, per-layer table (in-library HIP events) and the bench line.  Everything lands in
# $OUT (default out/; copy the summaries to profiles/).
cd "${GRAFT_REPO_ROOT:-.}"
export TMPDIR=/tmp
OUT=${OUT:-out}
mkdir -p $OUT/prof $OUT/pmc
TAG=${TAG:-r03}
# (kernel durations with the discriminator streams serialised, as in bench.py's roofline pass: concurrent kernels are each billed the shared time)
PCUDA_DSTREAMS=0 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o $TAG -- python3 bench.py --steps 3 --warmup 1 --no-cpu-baseline --no-roofline > $OUT/prof_bench_$TAG.log 2>&1
tail -1 $OUT/prof_bench_$TAG.log | cut -c1-300
F=$(find $OUT/prof -name "*kernel_stats.csv" | head -1)
[ -n "$F" ] && cp "$F" $OUT/${TAG}_kernel_stats.csv && head -12 "$F"
# (HBM traffic counters: scripts/gpu_pmc.sh, on single layers -- a --pmc pass over the whole step serialises
# thousands of dispatches and takes tens of minutes)
PCUDA_DSTREAMS=0 PCUDA_PROF_DUMP=$OUT/${TAG}_layers.csv python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $OUT/${TAG}_bench_prof.log 2>&1
python3 scripts/layer_table.py $OUT/${TAG}_layers.csv 60 > $OUT/${TAG}_layer_table.txt
tail -3 $OUT/${TAG}_layer_table.txt
python3 bench.py --full 2>/dev/null | tail -1 > $OUT/${TAG}_bench_line.json
cut -c1-200 $OUT/${TAG}_bench_line.json
