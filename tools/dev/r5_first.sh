#!/bin/bash
# Round 5, first GPU call: the suite, the x-error measurement, the --full bench line (with host_e2e).
#   usage: bash tools/dev/r5_first.sh OUTDIR
out=${1:?usage: r5_first.sh OUTDIR}
cd "$(dirname "$0")/../.." || exit 1
mkdir -p "$out"
timeout 900 python -m pytest tests -m gpu -x -q > "$out/r5_pytest.log" 2>&1; echo "pytest exit $?" >> "$out/r5_pytest.log"
tail -5 "$out/r5_pytest.log"
timeout 600 python tools/dev/r5_xerr.py > "$out/r5_xerr.log" 2>&1; cat "$out/r5_xerr.log"
timeout 900 python bench.py --full > "$out/r5_bench.json" 2> "$out/r5_bench.err"; echo "bench exit $?"
python - "$out/r5_bench.json" <<'PY'
import json, sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print("value",d["value"],"frac",d["roofline"]["frac"])
for k,v in d["config"]["summary"].items(): print(k, json.dumps(v))
PY
tail -3 "$out/r5_bench.err" | cut -c1-600
