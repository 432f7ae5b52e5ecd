#!/bin/bash
# One GPU visit: GPU test suite, then the full bench line, then the C3 run.  A step that times out ends the visit.
# Outputs: $OUT_DIR/<tag>_* (OUT_DIR defaults to run_out/).
set -o pipefail
out=${OUT_DIR:-run_out}
mkdir -p "$out"
tag=${1:-r2}
timeout -k 10 ${T_TESTS:-800} python -m pytest tests -m gpu -x -q > "$out/${tag}_tests.log" 2>&1
rc=$?
tail -5 "$out/${tag}_tests.log"
if [ $rc -eq 124 ] || [ $rc -eq 137 ]; then echo "tests timed out"; exit $rc; fi
timeout -k 10 300 python bench.py --full --steps 10 > "$out/${tag}_bench.json" 2> "$out/${tag}_bench.err"
rb=$?
echo "bench rc=$rb"; head -c 1500 "$out/${tag}_bench.json"
if [ $rb -eq 124 ] || [ $rb -eq 137 ]; then exit $rb; fi
timeout -k 10 300 python scripts/run_c3.py 50000000 4600000 0.005 0 0 0 31 auto > "$out/${tag}_c3.json" 2> "$out/${tag}_c3.err"
echo "c3 rc=$?"; cat "$out/${tag}_c3.json"; tail -3 "$out/${tag}_c3.err"
exit $rc
