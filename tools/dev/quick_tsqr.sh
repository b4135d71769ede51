# EKF kernel tests, the kernels alone (192 streams per launch, every launch timed), the single 4K stream and three default runs
# (bench lines with --full: per-kernel times and the Gram + Cholesky window).  Usage: tools/dev/quick_tsqr.sh <out dir>
OUT=${1:?usage: tools/dev/quick_tsqr.sh <out dir>}
mkdir -p "$OUT"
timeout -k 10 200 python -m pytest tests/test_gpu_kernels.py -k "ekf" -x -q > "$OUT/ekf_tests.log" 2>&1 || { tail -30 "$OUT/ekf_tests.log"; exit 1; }
tail -1 "$OUT/ekf_tests.log"
MSKF_BENCH_TIMING_PERIOD=1 timeout -k 5 90 python bench.py --full --no-cpu --steps 6 --warmup 2 --streams 192 --groups 1 --no-pipeline --gram-steps 0 > "$OUT/solo.json" 2> "$OUT/solo.err" || exit 1
python -c "import json,sys;d=json.load(open(sys.argv[1]));print('solo', round(d['value']), {k:round(x['avg_us']) for k,x in d['kernels'].items()}, d['checks_failed'])" "$OUT/solo.json"
timeout -k 5 120 python bench.py --full --config c5 --streams 1 --groups 1 --no-cpu --steps 20 --warmup 5 > "$OUT/c5_1.json" 2> "$OUT/c5_1.err" || exit 1
python -c "import json,sys;d=json.load(open(sys.argv[1]));print('c5 1 stream', round(d['value']), round(d['value_gram_cholesky']), {k:round(x['avg_us']) for k,x in d['kernels'].items()}, d['checks_failed'])" "$OUT/c5_1.json"
for rep in 1 2 3; do
  timeout -k 5 90 python bench.py --full --no-cpu --steps 20 --warmup 5 > "$OUT/d_$rep.json" 2> "$OUT/d_$rep.err" || exit 2
  python -c "import json,sys;d=json.load(open(sys.argv[1]));print('default rep$rep', round(d['value']), round(d['value_gram_cholesky']), d['host_phases_ms_per_step']['frames_completed_at_close_by_group'], {k:round(x['avg_us']) for k,x in d['kernels'].items() if 'ekf' in k}, d['checks_failed'])" "$OUT/d_$rep.json"
done
