#!/bin/bash
# HBM traffic of the blur kernel: separate --pmc passes (FETCH_SIZE and WRITE_SIZE do not fit one pass).
# usage: bash scratch/pmc_traffic.sh OUT_DIR   (from the repository root)
O=${1:?usage: pmc_traffic.sh OUT_DIR}
mkdir -p $O
rocprofv3 --kernel-trace --stats -d $O/trace --output-format csv -- python bench.py --full --steps 50 --warmup 5 --repeats 50 --no-cpu-baseline --no-train-step > $O/bench_under_rocprof.json 2> $O/trace.log
rocprofv3 --pmc FETCH_SIZE -d $O/fetch --output-format csv -- python scratch/prof_blur.py 5 > /dev/null 2>&1
rocprofv3 --pmc WRITE_SIZE -d $O/write --output-format csv -- python scratch/prof_blur.py 5 > /dev/null 2>&1
rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY -d $O/sq --output-format csv -- python scratch/prof_blur.py 5 > /dev/null 2>&1
find $O -name "*.csv" | head -20
