#!/bin/bash
# tools/profile_round.sh TAG DIR   (on the GPU box): the --full bench JSON + the three rocprofv3 passes the summaries are made from.
# Outputs under DIR: bench_TAG.json, prof_TAG_{stats,fetch,write}/ - DIR is the folder `python tools/summarize_prof.py TAG` reads (its docstring).
tag=${1:-r1}
out=${2:?usage: tools/profile_round.sh TAG DIR}
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
mkdir -p $out
python bench.py --full > $out/bench_$tag.json 2> $out/bench_$tag.err
tail -c 600 $out/bench_$tag.json; echo
B="python bench.py --steps 2 --warmup 1 --no-cpu-baseline --headline-only"
rm -rf $out/prof_${tag}_stats $out/prof_${tag}_fetch $out/prof_${tag}_write
rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof_${tag}_stats -o b -- $B > /dev/null 2>&1
rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $out/prof_${tag}_fetch -o b -- $B > /dev/null 2>&1
rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $out/prof_${tag}_write -o b -- $B > /dev/null 2>&1
find $out/prof_${tag}_* -name "*.csv" | head -20
# keep only what the summaries read (the traces are large)
find $out/prof_${tag}_* -type f ! -name "b_kernel_stats.csv" ! -name "b_counter_collection.csv" -delete
du -sh $out/prof_${tag}_*
