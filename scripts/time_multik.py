"""gk_map_add_graph_paths beside gk_graph_edge_coverage — the yardstick, in the same run — on C3's cleaned k = 31 graph
(scripts/run_c3.py: N x 150 bp reads over an E. coli-scale linear genome, deleteAll(<3), tips clipped, simplified): the contigs'
55-mers are added to a k = 55 table that holds the reads' counts, and the coverage of every edge of the same graph is taken from
its own k = 31 table.  One independent table access per window in both: a probe there, an update here; coverage reads both strands
of every edge, the add takes one strand per contig, so compare per window (coverage_windows, seeded["windows"]).
usage: python scripts/time_multik.py [reads=5000000] [genome=4600000] [err=0.005] [k1=31] [k2=55] [reps=3]
Prints one JSON line: both times (wall ms of the whole call, the minimum over the repetitions) and their ratio."""
import sys, time, json, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from genome_amd import synth
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.graph import buildGraph
from genome_amd.multik import clean

arg = lambda i, d, f=int: f(sys.argv[i]) if len(sys.argv) > i else d
n, G, err, k1, k2, reps = arg(1, 5_000_000), arg(2, 4_600_000), arg(3, 0.005, float), arg(4, 31), arg(5, 55), arg(6, 3)
L = 150
ctx = Context(0)
d = ctx.alloc(n * synth.record_stride(L) + 64)
ctx.synth_reads(d, n, L, "G", 3, 0, G, err)
m1 = HipDNAMap(ctx, k1, 0)
m1.count_reads_dev(d, n, L)
m1.deleteAll_lt(3)
g = buildGraph(k1, m1)
clean(g, m1, True, False)
g.simplifyGraph()
nodes, edges, length = g.counts()
out = {"reads": n, "genome": G, "err": err, "k1": k1, "k2": k2, "reps": reps, "graph": [nodes, edges, length]}
ms = {"gk_graph_edge_coverage": [], "gk_map_add_graph_paths": []}
for _ in range(reps):
    ctx.sync()
    t0 = time.perf_counter()
    cov = g.edgeCoverage(m1)
    ms["gk_graph_edge_coverage"].append(round((time.perf_counter() - t0) * 1e3, 3))
    m2 = HipDNAMap(ctx, k2, 0)
    m2.count_reads_dev(d, n, L)
    ctx.sync()
    t0 = time.perf_counter()
    st = m2.add_graph_paths(g, 3)
    ms["gk_map_add_graph_paths"].append(round((time.perf_counter() - t0) * 1e3, 3))
    out["distinct_after_seed"] = m2.size()
    m2.close()
out.update(ms=ms, coverage_windows=int(cov["kmers"].sum()), seeded=st,
           add_over_coverage=round(min(ms["gk_map_add_graph_paths"]) / min(ms["gk_graph_edge_coverage"]), 4))
print(json.dumps(out))
g.close(); m1.close(); ctx.free(d); ctx.close()
