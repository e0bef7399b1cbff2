# Round 5, call 5: the three tests that failed in call 4 (stale packs: an unreported load_state_dict -- now seen through the version
# counters) + the netcheck / ring files, then a quiet bench line.
# gpurun --timeout 900 -- 'bash scripts/gpu_r5e.sh r5e'
OUT=${OUT:-results}   # where the logs and JSON lines go
mkdir -p $OUT
export PYTHONDONTWRITEBYTECODE=1
export TMPDIR=/tmp
T=${1:-r5e}
O=$OUT/${T}_out.txt; : > $O
timeout 600 python -m pytest tests/test_gpu_net.py tests/test_gpu_parity2.py tests/test_gpu_steps.py tests/test_gpu_netcheck.py -m gpu -q --tb=short -p no:cacheprovider -k "same_weights or aser or netcheck or 4x4x1 or mir" > $OUT/${T}_tests.log 2>&1; echo "tests rc=$?" >> $O
timeout 400 python bench.py --full --gpus 1 --steps 20 --warmup 5 --no-cpu-baseline --no-accuracy > $OUT/${T}_bench.log 2>$OUT/${T}_bench.err; echo "bench rc=$?" >> $O
cat $O; grep -E "^FAILED|passed|failed|Error" $OUT/${T}_tests.log | tail -5
tail -1 $OUT/${T}_bench.log | python -c "
import json,sys
d=json.loads(sys.stdin.read()); a=d.get('also',{})
print(len(json.dumps(d)), json.dumps(dict(scr=d['ms_per_step'], repeats=d.get('ms_per_step_repeats'), roof=d.get('roofline',{}).get('frac'), aser=a.get('aser',{}).get('ms_per_step'), er=a.get('er',{}).get('ms_per_step'), mir=a.get('mir',{}).get('ms_per_step'), aser_l=a.get('aser',{}).get('roofline',{}).get('launches_per_step_all'))))"
