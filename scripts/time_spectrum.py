"""Time the count-spectrum pass (gk_map_spectrum) beside the read rate gk_dev_stream_bench reports in the same run.  Tables:

  c2      the headline's table after a C2 count (1M x 150 bp uniform reads, k = 31: 1.2e8 singletons in 12-byte slots)
  c3      C3's table before deleteAll (N x 150 bp reads over a 4.6 Mbp genome, 0.5 % errors, k = 31)
  spread  K keys with counts uniform in 1000..2000 (gk_map_add_counts: 16-byte slots are not involved, the table stays 12-byte)

For each: slots, bytes, the pass's wall ms (min and median of --reps calls; a call = memset of the device histogram, one kernel,
one read-back and wait), the ms the same bytes take at the measured read rate, and their ratio.  Prints one JSON object (and
writes it to --out).  GK_LIB_PATH selects the build of the library, as everywhere."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from genome_amd import synth  # noqa: E402
from genome_amd.dnamap import Context, HipDNAMap  # noqa: E402


def measure(ctx, m, reps, bins):
    st = m.stats()
    nbytes = st["slots"] * st["slot_bytes"]
    ms = []
    for _ in range(reps + 1):
        ctx.sync()
        t0 = time.perf_counter()
        s = m.spectrum(bins)
        ms.append((time.perf_counter() - t0) * 1e3)
    ms = sorted(ms[1:])                                   # (the first call takes its scratch from the device)
    rate = ctx.stream_bench(min(nbytes, 4 << 30), 10)["sum_GBps"]
    stream_ms = nbytes / (rate * 1e9) * 1e3
    live, bad, occ = m.verify()
    assert (s["distinct"], s["occurrences"]) == (live, occ) and bad == 0 and int(s["hist"].sum()) == live
    h = s["hist"]
    return {"slots": st["slots"], "slot_bytes": st["slot_bytes"], "table_bytes": nbytes, "distinct": s["distinct"], "max_count": s["max_count"],
            "singletons": int(h[1]), "overflow_bin": int(h[-1]), "bins": bins, "pass_ms_min": round(ms[0], 4), "pass_ms_median": round(ms[len(ms) // 2], 4),
            "stream_read_GBps": round(rate, 1), "stream_ms_same_bytes": round(stream_ms, 4), "ratio_pass_over_stream": round(ms[0] / stream_ms, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c2,c3,spread")
    ap.add_argument("--c3-reads", type=int, default=5_000_000)
    ap.add_argument("--spread-keys", type=int, default=40_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--bins", type=int, default=4096)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    k, L = 31, 150
    ctx = Context(0)
    res = {"lib": os.path.basename(os.environ.get("GK_LIB_PATH", "libgenome_amd.so")), "k": k}
    for case in args.cases.split(","):
        if case == "c2":
            n = 1_000_000
            d = ctx.alloc(n * synth.record_stride(L) + 64)
            ctx.synth_reads(d, n, L, "U", 2, 0, 5_000_000, 0.01)
            m = HipDNAMap(ctx, k, int(n * (L - k + 1) * 1.05))
            m.count_reads_dev(d, n, L)
            ctx.free(d)
        elif case == "c3":
            n = args.c3_reads
            d = ctx.alloc(n * synth.record_stride(L) + 64)
            ctx.synth_reads(d, n, L, "G", 3, 0, 4_600_000, 0.005)
            m = HipDNAMap(ctx, k, 0)
            m.count_reads_dev(d, n, L)
            ctx.free(d)
        else:
            n = args.spread_keys
            rng = np.random.default_rng(7)
            lo = np.unique(rng.integers(0, 1 << 62, n, dtype=np.uint64))
            m = HipDNAMap(ctx, k, len(lo))
            step = 1 << 23
            for a in range(0, len(lo), step):
                part = lo[a:a + step]
                m.add_counts(part, np.zeros(len(part), np.uint64), rng.integers(1000, 2001, len(part)).astype(np.int32))
        res[case] = measure(ctx, m, args.reps, args.bins)
        m.close()
        ctx.trim()
    ctx.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
