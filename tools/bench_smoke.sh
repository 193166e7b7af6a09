#!/bin/bash
# the default bench line, its kernel trace, and smoke(): tools/bench_smoke.sh <tag>
set -o pipefail
out=gpurun_out/$1; mkdir -p $out; export TMPDIR=/tmp
timeout -k 10 400 python -u bench.py --full > $out/bench.json 2> $out/bench.err || { tail -20 $out/bench.err; exit 1; }
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof -o run -- python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-pmc > $out/prof_bench.json 2> $out/prof.err || { tail -20 $out/prof.err; exit 1; }
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $out/smoke.log 2>&1 || { tail $out/smoke.log; exit 1; }
tail -1 $out/smoke.log
