# parity mode at positions 1 858..1 921: the bench line with per-class kernel times, then a rocprofv3 kernel trace; both go to $BENCH_OUT (default <repo>/bench_out/)
repo=$(cd "$(dirname "$0")/.." && pwd); out=${BENCH_OUT:-$repo/bench_out}; mkdir -p "$out"
cd /tmp && export TMPDIR=/tmp
python3 $repo/bench.py --full --pos0 1850 --steps 64 --warmup 8 --mode parity --no-cpu-baseline --no-other-configs --no-prefill --no-sampled --no-by-position --no-trait-ops > $out/long_parity.json 2> $out/long_parity.err
rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/lp -o lp -- python3 $repo/bench.py --pos0 1850 --steps 32 --warmup 4 --graph 0 --mode parity --no-cpu-baseline --no-kprof --no-other-configs --no-prefill --no-sampled --no-by-position --no-trait-ops > /dev/null 2>&1
cp $(find /tmp/lp -name "*kernel_stats.csv" | head -1) $out/long_parity_kernel_stats.csv
