# A/B of the variance GEMM's tilings on the headline workload: bash tools/ab_tilings.sh "0 256 257 258"  (option "swizzle" values)
set -e
AB_DIR=${AB_DIR:-ab_results}
mkdir -p $AB_DIR
for s in ${1:-0 256 257 258}; do
  python bench.py --steps 5 --warmup 2 --full --no-cpu-baseline --option swizzle=$s > $AB_DIR/s$s.json 2>$AB_DIR/s$s.err
  python - <<PY
import json
d=json.loads(open("$AB_DIR/s$s.json").read().strip().splitlines()[-1])
print($s, d["ms_per_step"], d["roofline"]["frac"], flush=True)
PY
done
