# round 4: the bench line (driver's command) + profile bundle once more, on another lease.   gpurun --timeout 1500 -- 'bash scripts/gpu_r4y.sh r4y'
OUT=${OUT:-results}   # where the logs and JSON lines go
mkdir -p $OUT
export PYTHONDONTWRITEBYTECODE=1
export TMPDIR=/tmp
T=${1:-r4y}
rocm-smi --showclocks --showpower 2>&1 | grep -E "sclk|mclk|fclk|Power" | head -6 > $OUT/${T}_smi.txt
timeout 1200 python bench.py --full --gpus 1 --steps 20 --warmup 5 > $OUT/${T}_bench_scr.log 2>$OUT/${T}_bench_scr.err; echo "bench rc=$?"
tail -1 $OUT/${T}_bench_scr.log | cut -c1-700
bash scripts/gpu_prof.sh $T
