"""gk_graph_build_cycles beside gk_graph_build — the yardstick, in the same run — on C3's table (scripts/run_c3.py: N x 150 bp reads
over an E. coli-scale linear genome, k = 31, deleteAll(<3)): (a) as it is, which holds no perfect cycle, so the difference is the
cost of asking (one census pass); (b) with 100 circular replicons of 5 to 50 kbases planted (error-free 150 bp reads tiled around
each, stride 30, so every k-mer passes the filter), where the members are found, their minima taken and the arcs appended.
usage: python scripts/time_cycles.py [reads=5000000] [genome=4600000] [err=0.005] [k=31] [reps=3] [replicons=100]
Prints one JSON line."""
import sys, time, json, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from genome_amd import synth
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.graph import buildGraph

arg = lambda i, d, f=int: f(sys.argv[i]) if len(sys.argv) > i else d
n, G, err, k, reps, nrep = arg(1, 5_000_000), arg(2, 4_600_000), arg(3, 0.005, float), arg(4, 31), arg(5, 3), arg(6, 100)
L = 150
ctx = Context(0)
d = ctx.alloc(n * synth.record_stride(L) + 64)
ctx.synth_reads(d, n, L, "G", 3, 0, G, err)


def timed(m):
    """-> ({name: [ms per rep]}, counts of the plain graph, counts and stats of the keeping one), the two builds alternating"""
    ms = {"gk_graph_build": [], "gk_graph_build_cycles": []}
    plain = kept = stats = None
    for _ in range(reps):
        for name, keep in (("gk_graph_build", False), ("gk_graph_build_cycles", True)):
            ctx.sync()
            t0 = time.perf_counter()
            g = buildGraph(k, m, keep_cycles=keep)
            ms[name].append(round((time.perf_counter() - t0) * 1e3, 3))
            if keep:
                kept, stats = list(g.counts()), g.cycleStats()
            else:
                plain = list(g.counts())
            g.close()
    return ms, plain, kept, stats


def planted(rng):
    """.bin records of error-free reads tiled around `nrep` random circular sequences of 5 to 50 kbases"""
    recs, total = [], 0
    for _ in range(nrep):
        length = int(rng.integers(5_000, 50_001))
        seq = rng.integers(0, 4, length, dtype=np.uint8)
        ext = np.concatenate([seq, seq[:L - 1]])
        starts = np.arange(0, length, 30)
        recs.append(synth.pack_reads(ext[starts[:, None] + np.arange(L)[None, :]]))
        total += length
    return np.concatenate(recs), total


out = {"reads": n, "genome": G, "err": err, "k": k, "reps": reps}
m = HipDNAMap(ctx, k, 0)
m.count_reads_dev(d, n, L)
m.deleteAll_lt(3)
out["good_kmers"] = m.size()
ms, plain, kept, stats = timed(m)
out["no_cycles"] = {"ms": ms, "graph": plain, "graph_cycles": kept, "stats": stats,
                    "cycles_over_build": round(min(ms["gk_graph_build_cycles"]) / min(ms["gk_graph_build"]), 4)}
m.close()
rec, bases = planted(np.random.default_rng(7))
m = HipDNAMap(ctx, k, 0)
m.count_reads_dev(d, n, L)
m.count_reads(rec.tobytes(), len(rec))
m.deleteAll_lt(3)
ms, plain, kept, stats = timed(m)
out["planted"] = {"replicons": nrep, "bases": bases, "good_kmers": m.size(), "ms": ms, "graph": plain, "graph_cycles": kept, "stats": stats,
                  "cycles_over_build": round(min(ms["gk_graph_build_cycles"]) / min(ms["gk_graph_build"]), 4)}
print(json.dumps(out))
m.close(); ctx.free(d); ctx.close()
