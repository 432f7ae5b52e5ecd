"""One gk_graph_remove_weak_edges round beside one gk_graph_clip_tips round, on C3's graph (scripts/run_c3.py: N x 150 bp reads over
an E. coli-scale genome, k = 31) after deleteAll(<3) + buildGraph: each round on a fresh graph of the same table, in the same run.
The expectation to confirm or refute: both calls compute the coverage of every live edge and build the in-edge lists, and differ
in one mark kernel, so they cost about the same.
usage: python scripts/time_weak_edges.py [reads=5000000] [genome=4600000] [err=0.005] [k=31] [reps=3] [ratio=5] [floor=0]
Prints one JSON line."""
import sys, time, json, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from genome_amd import synth
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.graph import buildGraph

arg = lambda i, d, f=int: f(sys.argv[i]) if len(sys.argv) > i else d
n, G, err, k, reps, ratio, floor = arg(1, 5_000_000), arg(2, 4_600_000), arg(3, 0.005, float), arg(4, 31), arg(5, 3), arg(6, 5), arg(7, 0)
L = 150
ctx = Context(0)
d = ctx.alloc(n * synth.record_stride(L) + 64)
ctx.synth_reads(d, n, L, "G", 3, 0, G, err)
m = HipDNAMap(ctx, k, 0)
m.count_reads_dev(d, n, L)
m.deleteAll_lt(3)
good = m.size()
clip_ms, weak_ms = [], []
for rep in range(reps):
    g = buildGraph(k, m)
    ctx.sync()
    t0 = time.perf_counter(); tips = g.clipTips(m); clip_ms.append((time.perf_counter() - t0) * 1e3)
    g.close()
    g = buildGraph(k, m)
    nodes, edges, length = g.counts()
    ctx.sync()
    t0 = time.perf_counter(); stats = g.removeWeakEdges(m, None, ratio, floor); weak_ms.append((time.perf_counter() - t0) * 1e3)
    after = list(g.counts())
    g.close()
print(json.dumps({"reads": n, "genome": G, "err": err, "k": k, "good_kmers": good, "graph": [nodes, edges, length], "max_len": 2 * k, "ratio": ratio,
                  "floor": floor, "weak": stats, "tips_removed": tips, "remove_weak_ms": [round(x, 3) for x in weak_ms],
                  "clip_tips_ms": [round(x, 3) for x in clip_ms], "weak_over_clip": round(min(weak_ms) / min(clip_ms), 3), "graph_after_weak": after}))
m.close(); ctx.free(d); ctx.close()
