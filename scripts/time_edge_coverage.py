"""gk_graph_edge_coverage over all edges, and one gk_graph_clip_tips round, on C3's graph (scripts/run_c3.py: N x 150 bp reads over
an E. coli-scale genome, k = 31) after deleteAll(<3) + buildGraph, beside the yardstick from the same run: the unitig walk of
gk_graph_build (phases unitig_measure + unitig_emit: k_walk_q + k_place_edges), which makes about as many table probes.
usage: python scripts/time_edge_coverage.py [reads=5000000] [genome=4600000] [err=0.005] [k=31] [reps=3]
Prints one JSON line."""
import sys, time, json, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from genome_amd import synth
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.graph import buildGraph

arg = lambda i, d, f=int: f(sys.argv[i]) if len(sys.argv) > i else d
n, G, err, k, reps = arg(1, 5_000_000), arg(2, 4_600_000), arg(3, 0.005, float), arg(4, 31), arg(5, 3)
L = 150
ctx = Context(0)
d = ctx.alloc(n * synth.record_stride(L) + 64)
ctx.synth_reads(d, n, L, "G", 3, 0, G, err)
m = HipDNAMap(ctx, k, 0)
m.count_reads_dev(d, n, L)
m.deleteAll_lt(3)
good = m.size()
g = buildGraph(k, m)
nodes, edges, length = g.counts()
bs = g.buildStats()
walk_ms = bs["phase_ms"]["unitig_measure"] + bs["phase_ms"]["unitig_emit"]
ids = np.arange(g.idBounds()[1], dtype=np.uint32)
cov_ms = []
for _ in range(reps):
    ctx.sync()
    t0 = time.perf_counter(); c = g.edgeCoverage(m, ids); cov_ms.append((time.perf_counter() - t0) * 1e3)
lens = c["kmers"][c["kmers"] > 0] - 1
t0 = time.perf_counter(); removed = g.clipTips(m); clip_ms = (time.perf_counter() - t0) * 1e3
probes = int(c["kmers"].sum())
print(json.dumps({"reads": n, "genome": G, "err": err, "k": k, "good_kmers": good, "graph": [nodes, edges, length], "probes": probes,
                  "long_edges": int((lens >= 64).sum()), "windows_on_long_edges": int((lens[lens >= 64] + 1).sum()), "longest_edge": int(lens.max()) if len(lens) else 0,
                  "missing": c["missing"], "walk_phase_ms": round(walk_ms, 3), "build_phase_ms": {a: round(b, 3) for a, b in bs["phase_ms"].items()},
                  "edge_coverage_ms": [round(x, 3) for x in cov_ms], "edge_coverage_over_walk": round(min(cov_ms) / walk_ms, 3) if walk_ms else None,
                  "probes_per_s": round(probes / (min(cov_ms) * 1e-3), 1), "clip_tips_ms": round(clip_ms, 3), "tips_removed": removed,
                  "graph_after_clip": list(g.counts())}))
g.close(); m.close(); ctx.free(d); ctx.close()
