#!/bin/bash
# One GPU visit: the full bench line + rocprofv3 kernel stats + PMC passes (separate passes, per the guide) for the default
# bench workload.  Outputs under $OUT_DIR/<tag>_* (OUT_DIR defaults to run_out/ in the repository; scripts/summarize_pmc.py
# reads the same folder and copies what matters into profiles/).
R=$(cd "$(dirname "$0")/.." && pwd); out=${OUT_DIR:-$R/run_out}; tag=${1:-r01}; path=${2:-auto}
export TMPDIR=/tmp; mkdir -p "$out"
python3 $R/bench.py --full --steps 10 --warmup 2 --no-extras --insert-path $path > $out/${tag}_bench.json 2> $out/${tag}_bench.err
cd /tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $out/${tag}_stats -- python3 $R/bench.py --steps 10 --warmup 2 --no-cpu-baseline --no-extras --insert-path $path > $out/${tag}_stats.log 2>&1
rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $out/${tag}_pmc_fetch -- python3 $R/bench.py --steps 3 --warmup 1 --no-cpu-baseline --no-extras --insert-path $path > $out/${tag}_pmc_fetch.log 2>&1
rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $out/${tag}_pmc_write -- python3 $R/bench.py --steps 3 --warmup 1 --no-cpu-baseline --no-extras --insert-path $path > $out/${tag}_pmc_write.log 2>&1
rocprofv3 --pmc TCC_EA0_RDREQ_sum TCC_EA0_WRREQ_sum TCC_EA0_ATOMIC_sum --kernel-trace --output-format csv -d $out/${tag}_pmc_req -- python3 $R/bench.py --steps 3 --warmup 1 --no-cpu-baseline --no-extras --insert-path $path > $out/${tag}_pmc_req.log 2>&1
cat $out/${tag}_bench.json | cut -c1-300
