#!/bin/bash
# the whole GPU suite, then the bench line
R=$PWD; OUT=$R/gpurun_out/${1:-suite}; mkdir -p $OUT
timeout -k 10 1100 python3 -m pytest tests -x -q -m gpu > $OUT/suite.log 2>&1
rc=$?; echo "[suite] rc=$rc"; tail -4 $OUT/suite.log
[ $rc -eq 0 ] || exit 1
timeout -k 10 600 python3 bench.py --full --steps 20 --warmup 5 > $OUT/bench.json 2> $OUT/bench.err
echo "[suite] bench rc=$?"; python3 tools/show_bench.py $OUT/bench.json | cut -c1-900
