#!/bin/bash
# the full bench line of the current tree:  scripts/r06/gpu_bench.sh <output dir>
out=${1:?usage: gpu_bench.sh <output dir>}
root=${GRAFT_REPO_ROOT:-$(pwd)}
cd $root; mkdir -p "$out"
( time python bench.py --full ) > "$out/bench_default.txt" 2>&1
grep '^{"metric' "$out/bench_default.txt" | tail -1 > "$out/bench_default.json"
python - "$out/bench_default.json" <<'PY'
import json, sys
d=json.loads(open(sys.argv[1]).read())
print('value', d['value'], 'ms', d['ms_per_step'])
print('deblur', {k:v for k,v in d['deblur'].items() if 'ms' in k or k=='unchanged_caller'})
print('flow', {k:v for k,v in d['get_flow'].items() if 'ms' in k})
print('train', {k:v for k,v in d['train_iteration'].items() if 'ms' in k or k=='unchanged_caller'})
print('repeat', d['repeat']['ms_per_step'], d['repeat']['forward_only_no_grad']['ms_per_render'])
print('dyn3', d['dynamic_config3']['ms_per_step'])
print('roofline', {k:v for k,v in d['roofline'].items() if k in ('achieved','frac','avg_kernel_ms','kernel')})
PY
tail -3 "$out/bench_default.txt" | cut -c1-300
