"""Wall times of the collective count of a host `.bin` stream (gk_dist_count_reads) at world 1 over RCCL, against the one-rank
gk_map_count_reads of the same stream; and the super-k-mer route in its two framings on the same uniform reads (host_ragged = 1
forces the offset-framed route).  Loads the TEST build of the library (the host_ragged switch).  The route kernels' own times
come from running `framing` under `rocprofv3 --kernel-trace --stats`: k_skm_route<16, false> is the fixed-stride route,
k_skm_route<16, true> the offset-framed one, with the same number of calls over the same reads.

  python scripts/time_dist_bin.py [all|framing] [nreads]     C2-sized by default: 10^6 reads of a 5 Mbp genome (1 % errors),
                                                             k = 31, mates cut at a random length 0..150 for the ragged stream
Prints one JSON line per case: median and min wall ms over 5 timed calls after one warm-up, each into a fresh map."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GK_LIB_PATH", os.path.join(ROOT, "genome_amd", "libgenome_amd_test.so"))

import numpy as np  # noqa: E402

from genome_amd import synth  # noqa: E402
from genome_amd.dist import DistDNAMap, HipDist, unique_id  # noqa: E402
from genome_amd.dnamap import Context, HipDNAMap  # noqa: E402

K, L, REPS = 31, 150, 5


def ragged_from(rec: np.ndarray, seed: int = 7) -> bytes:
    """every record cut at a random length 0..L: [len][ceil(len/4) bytes], the unused bits of the last byte cleared"""
    n = rec.shape[0]
    lens = np.random.default_rng(seed).integers(0, L + 1, n)
    keep = 1 + (lens + 3) // 4
    out = rec.copy()
    out[:, 0] = lens
    last = keep - 1                                        # column of the last data byte (0 = none)
    rows = np.flatnonzero(last > 0)
    tail = lens[rows] % 4
    mask = np.where(tail == 0, 0xFF, (1 << (2 * tail)) - 1).astype(np.uint8)
    out[rows, last[rows]] &= mask
    cols = np.arange(rec.shape[1])[None, :]
    return out[cols < keep[:, None]].tobytes()


def timed(f):
    f()
    ms = []
    for _ in range(REPS):
        ms.append(f())
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(min(ms)), 3)}


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
    ctx = Context(0)
    hd = HipDist(ctx, 0, 1, unique_id())
    rec = synth.reads_mode_g(n, L, 5_000_000, 0.01, config_id=2)
    uniform = rec.tobytes()
    ragged = ragged_from(rec)
    cap = n * (L - K + 1) // 4

    def one_rank(b):
        def f():
            m = HipDNAMap(ctx, K, cap)
            ctx.sync()
            t0 = time.perf_counter()
            m.count_reads(b, n)
            ctx.sync()
            t = (time.perf_counter() - t0) * 1e3
            m.close()
            return t
        return f

    def dist(b, host_ragged=0):
        def f():
            ctx.set_option("host_ragged", host_ragged)
            pm = DistDNAMap(hd, K, cap)
            ctx.sync()
            t0 = time.perf_counter()
            sent, owned = pm.count_reads(b, n)
            ctx.sync()
            t = (time.perf_counter() - t0) * 1e3
            assert sent == owned
            pm.close()
            ctx.set_option("host_ragged", 0)
            return t
        return f

    cases = []
    if what == "all":
        cases += [("ragged", "gk_map_count_reads", one_rank(ragged)), ("ragged", "gk_dist_count_reads", dist(ragged))]
    cases += [("uniform", "gk_dist_count_reads fixed-stride route", dist(uniform, 0)),
              ("uniform", "gk_dist_count_reads offset-framed route (host_ragged)", dist(uniform, 1))]
    for stream, call, f in cases:
        b = ragged if stream == "ragged" else uniform
        print(json.dumps({"stream": stream, "reads": n, "bytes": len(b), "k": K, "world": 1, "call": call, **timed(f)}), flush=True)
    hd.close(); ctx.close()


if __name__ == "__main__":
    main()
