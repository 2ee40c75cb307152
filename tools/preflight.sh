#!/bin/bash
# The end-of-round check in one GPU session:   bash tools/preflight.sh OUTDIR
#   smoke() on cuda:0, the -m gpu suite, the full bench line (bench.py --full) -> OUTDIR/preflight_*.{txt,json,err}
OUT=${1:?usage: bash tools/preflight.sh OUTDIR}
mkdir -p "$OUT" && OUT=$(cd "$OUT" && pwd) || exit 1
cd "$(dirname "$0")/.."
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -1
timeout 1200 python -m pytest tests -m gpu -x -q > "$OUT/preflight_tests.txt" 2>&1; echo "pytest rc=$? $(tail -1 "$OUT/preflight_tests.txt")"
python bench.py --full > "$OUT/preflight_bench.json" 2> "$OUT/preflight_bench.err"; echo "bench rc=$?"
python - "$OUT/preflight_bench.json" <<'PY'
import json
import sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
a = d['also']
print('ms/step %.3f  clouds/s %.0f  roofline %.3f (%.1f TFLOP/s-eq, %.2f ms of families)  best %.3f  whole-step %.1f TFLOP/s  cfg2 %.2f ms  published %.2f ms  '
      'dgcnn %.2f ms  cfg5-shape %.2f ms  cpu %.1f clouds/s' % (
          d['ms_per_step'], d['value'], d['roofline']['frac'], d['roofline']['achieved'], d['roofline']['ms_per_step'],
          d['roofline_best']['frac'], d['whole_step'].get('achieved', 0.0), a['cfg2']['ms_per_step'],
          a['published_variant']['ms_per_step'], a['dgcnn']['ms_per_step'], a['cfg5_shape']['ms_per_step'], d['cpu_baseline']['value']))
PY
