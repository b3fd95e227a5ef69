#!/bin/bash
# regenerate the judged artefacts under $BENCH_OUT (default bench_out/; copy into profiles/ afterwards)
cd /tmp; export TMPDIR=/tmp; cd $GRAFT_REPO_ROOT
O=${BENCH_OUT:-bench_out}; mkdir -p $O
python bench.py --full > $O/bench.json 2> $O/bench.err
tail -c 3000 $O/bench.json
rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/ks -o ks -- python bench.py --full --steps 4 --warmup 2 --no-cpu-baseline > /dev/null 2>&1
cp /tmp/ks/ks_kernel_stats.csv $O/bench_kernel_stats.csv
head -12 $O/bench_kernel_stats.csv | cut -c1-160
