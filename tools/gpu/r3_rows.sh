O=${AVEC_OUT:-$PWD/out}; mkdir -p $O
cd $GRAFT_REPO_ROOT
python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline 2>/dev/null | grep "^{" > $O/r3_rows.json
python - "$O/r3_rows.json" <<'PY'
import json, sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(d['ms_per_step'])
for x in d['roofline']['rows']: print(x['kernel'], x['launches_per_step'], x['avg_us'], x['tflops'])
for k,v in d['roofline']['families'].items(): print(k, v)
PY
