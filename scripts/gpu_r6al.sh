# Round 6 (experiment): the ASER update's one synchronisation as a poll of the event (OCL_ASER_SPIN=1) instead of a blocking wait.
OUT=${OUT:-results}   # where the logs and JSON lines go
T=${1:-r6al}
mkdir -p $OUT
run() {  # workload, label, env...
  wl=$1; lab=$2; shift 2
  env "$@" timeout -k 10 300 python bench.py --full --workload $wl --steps 100 --warmup 5 --no-roofline --no-accuracy --no-cpu-baseline --no-also > $OUT/${T}_${wl}_${lab}.json 2> $OUT/${T}_${wl}_${lab}.err
  python - $wl "$lab" $OUT/${T}_${wl}_${lab}.json <<'PY'
import json,sys
d=json.loads([l for l in open(sys.argv[3]) if l.startswith("{")][-1])
print(sys.argv[1], sys.argv[2], "ms_per_step %.4f max %.4f" % (d["ms_per_step"], d.get("ms_per_step_max",0)), d["ms_per_step_repeats"])
PY
}
{
run aser blocking X=1
run aser spin OCL_ASER_SPIN=1
run aser blocking X=1
run aser spin OCL_ASER_SPIN=1
run aser blocking X=1
run aser spin OCL_ASER_SPIN=1
} 2>&1 | tee $OUT/${T}_aser_spin_ab.txt
