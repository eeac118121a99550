#!/bin/bash
# packed-row GEMM microbench + pack tests + short bench
set -o pipefail
O=${OUT:-out}; mkdir -p $O
export PYTHONUNBUFFERED=1
timeout -k 10 300 python -u tools/gemm_live_bench.py > $O/live_gemm.log 2>&1 &&
timeout -k 10 600 python -u -m pytest tests/test_pack_gpu.py tests/test_bench_shape_gpu.py tests/test_kernels_gpu.py -x -q --timeout 240 --timeout-method thread > $O/live_tests.log 2>&1 &&
timeout -k 10 600 python -u bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-decode --sweep "" > $O/live_bench.log 2>&1
rc=$?
cat $O/live_gemm.log | grep -v amdgpu.ids
tail -3 $O/live_tests.log
tail -c 1500 $O/live_bench.log
exit $rc
