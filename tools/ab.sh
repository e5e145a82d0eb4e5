#!/bin/bash
# A/B the variants/libart_<name>.so builds on the GPU box: one bench line each (no CPU baseline).
#   bash tools/ab.sh name1 name2 ...   [extra bench args in $AB_ARGS; logs under $AB_OUT, default ab_out]
set -euo pipefail
out=${AB_OUT:-ab_out}
mkdir -p "$out"
for v in "$@"; do
  ART_LIB=$PWD/variants/libart_$v.so timeout -k 10 240 python bench.py --full --no-cpu-baseline --frames 3 ${AB_ARGS:-} > "$out/$v.log" 2>&1
  python3 -c "import json,sys; d=json.loads(open('$out/$v.log').read().strip().splitlines()[-1]); print('$v', '%.1f Gt/s'%(d['value']/1e9), 'rt %.4f ms'%d['kernel_ms']['raytrace'], 'perm %.4f'%d['kernel_ms']['permeate'])"
done
