#!/bin/bash
# Three default bench.py runs on one box (A/B of a code change needs the same box: boxes differ by +-3 %).
python3 -c "import torch"
line=$(mktemp)
for i in 1 2 3; do
  timeout -s KILL 300 python3 bench.py --full --cpu-seconds 0 > "$line" 2>/dev/null
  python3 -c "
import json, sys; d=json.load(open(sys.argv[1])); print(d['value'], d['ms_per_step'], d['roofline']['frac'], {k: round(v['avg_us']) for k, v in d['kernels'].items()})" "$line"
done
rm -f "$line"
