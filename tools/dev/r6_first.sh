#!/bin/bash
# Round 6, first GPU call on the new bench / ring / pinned-extent code: the new tests, the --full bench line (timed), launch shapes.
#   usage: bash tools/dev/r6_first.sh OUTDIR
out=${1:?usage: r6_first.sh OUTDIR}
export TMPDIR=/tmp EICOS_EXPERIMENT=1
cd "$(dirname "$0")/../.." || exit 1; mkdir -p "$out"
{ timeout 900 python -m pytest tests -m gpu -x -q -k "ring_of_events or partly_pinned or contract_json or host_pointer" 2>&1 | tail -8
time python bench.py --full > "$out/r6_bench.json" 2> "$out/r6_bench.err"
} > "$out/r6_first.log" 2>&1
cat "$out/r6_first.log" | cut -c1-250
