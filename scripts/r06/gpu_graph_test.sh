#!/bin/bash
# the graphed-iteration tests, then the full bench line:  scripts/r06/gpu_graph_test.sh <output dir>
out=${1:?usage: gpu_graph_test.sh <output dir>}
root=${GRAFT_REPO_ROOT:-$(pwd)}
cd $root; mkdir -p "$out"
timeout 900 python -X faulthandler -m pytest tests/test_gpu_graphed.py -x -q -m gpu 2>&1 | grep -v "^  \|Warning\|^$" | tail -8
( time python bench.py --full --steps 20 --warmup 5 ) > "$out/bench.txt" 2>&1
grep '^{"metric' "$out/bench.txt" | tail -1 > "$out/bench.json"
python - "$out/bench.json" <<'PY'
import json, sys
d=json.loads(open(sys.argv[1]).read())
print('value', d['value'], 'ms', d['ms_per_step'])
print('train', {k:v for k,v in d['train_iteration'].items() if 'ms' in k or k=='graphed'})
print('small', d.get('reference_operating_point'))
print('roofline', {k:v for k,v in d['roofline'].items() if k in ('achieved','frac','avg_kernel_ms','kernel','algorithmic_bytes_formula')})
PY
tail -4 "$out/bench.txt" | cut -c1-200
