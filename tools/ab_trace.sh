#!/bin/bash
# A/B of library variants: kernel-trace stats of a short bench run per variant (ART_LIB), plus the
# bench's ms/step.  bash tools/ab_trace.sh <config> <variant|base>...
set -euo pipefail
cfg=$1; shift
export TMPDIR=/tmp
for v in "$@"; do
  out=gpurun_out/ab/$v
  mkdir -p "$out"
  lib=$PWD/audio-raytracer_amd/lib/libart.so
  [ "$v" != base ] && lib=$PWD/variants/libart_$v.so
  ART_LIB=$lib timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d "$out/trace" -o run -- python3 bench.py --full --config $cfg --no-cpu-baseline --no-dynamic --frames 5 --steps 50 > "$out/trace.log" 2>&1
  echo "== $v"
  python3 tools/kstats.py "$out/trace/run_kernel_stats.csv" > "$out/kstats.txt"; sed -n 1,8p "$out/kstats.txt"
  ART_LIB=$lib timeout -k 10 200 python bench.py --full --config $cfg --no-cpu-baseline --no-dynamic --frames 5 > "$out/bench.log" 2>&1
  tail -1 "$out/bench.log" | python3 -c "import json,sys; r=json.loads(sys.stdin.read()); print('ms_per_step %.4f stage %.4f' % (r['ms_per_step'], r['kernel_ms']['raytrace']))"
done
