#!/bin/bash
# rocprofv3 kernel-trace stats of the full bench.py command (--full: the int8 region and the Metropolis sub-benchmark included);
# the CSV summary and the bench line land in $OUT/TAG (OUT defaults to profile_out under the repo root).
# usage (on the GPU box, from the repo root): tools/profile_bench.sh TAG
TAG=${1:-r01}
R=$PWD
O=$R/${OUT:-profile_out}/$TAG
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $O -o $TAG -- python $R/bench.py --full --no-cpu-baseline --steps 3 --warmup 1 > $O/bench.json 2> $O/bench.err < /dev/null
cd $R
find $O -name "*kernel_stats.csv" | head -1 | xargs -r head -14
find $O -name "*kernel_trace.csv" -delete
du -sh $O
