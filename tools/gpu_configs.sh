# bench lines for the other BASELINE configs (c3 stereo 24-bit, c4 chunked 1e8 blocks, c5 fixed-only)
# Usage: [OUT=<output directory, default bench_out>] bash tools/gpu_configs.sh
set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 300 python bench.py --full --config c5 --steps 5 --warmup 2 --cpu-seconds 5 > $OUT/bench_c5.json 2> $OUT/bench_c5.err || { tail $OUT/bench_c5.err; exit 1; }
echo c5; cat $OUT/bench_c5.json
timeout -k 10 400 python bench.py --full --config c3 --steps 3 --warmup 1 --cpu-seconds 5 > $OUT/bench_c3.json 2> $OUT/bench_c3.err || { tail $OUT/bench_c3.err; exit 1; }
echo c3; cat $OUT/bench_c3.json
timeout -k 10 400 python bench.py --full --config c4 --steps 2 --warmup 1 --cpu-seconds 0 > $OUT/bench_c4.json 2> $OUT/bench_c4.err || { tail $OUT/bench_c4.err; exit 1; }
echo c4; cat $OUT/bench_c4.json
