"""One gk_graph_pop_bubbles round beside one gk_graph_clip_tips round, on C3's graph (scripts/run_c3.py: N x 150 bp reads over an
E. coli-scale genome, k = 31) after deleteAll(<3) + buildGraph: each round on a fresh graph of the same table, in the same run.
The expectation to confirm or refute: pop computes coverage for the candidate edges only, clip for every edge, so pop costs less.
usage: python scripts/time_pop_bubbles.py [reads=5000000] [genome=4600000] [err=0.005] [k=31] [reps=3]
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
clip_ms, pop_ms, dist_ms = [], [], []
for rep in range(reps):
    g = buildGraph(k, m)
    ctx.sync()
    t0 = time.perf_counter(); tips = g.clipTips(m); clip_ms.append((time.perf_counter() - t0) * 1e3)
    g.close()
    g = buildGraph(k, m)
    nodes, edges, length = g.counts()
    # the candidate edges, on the host from the by-id export: live, within 2k, sharing (start, end) with another such edge
    e = g.edgesById(np.arange(g.idBounds()[1], dtype=np.uint32))
    ok = e["alive"] & (e["len"] <= 2 * k)
    key = (e["start"][ok].astype(np.uint64) << np.uint64(32)) | e["end"][ok].astype(np.uint64)
    _u, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    cand_ids = np.nonzero(ok)[0][cnt[inv] >= 2].astype(np.uint32)
    # the distance kernel alone, on all ordered pairs of candidates that share both ends (a superset of what the round compares)
    order = np.argsort(key[cnt[inv] >= 2], kind="stable")
    a, b = cand_ids[order][:-1], cand_ids[order][1:]
    same = np.sort(key[cnt[inv] >= 2])[:-1] == np.sort(key[cnt[inv] >= 2])[1:]
    ctx.sync()
    t0 = time.perf_counter(); dist = g.edgeDistance(a[same], b[same], 3); dist_ms.append((time.perf_counter() - t0) * 1e3)
    ctx.sync()
    t0 = time.perf_counter(); removed, pairs = g.popBubbles(m); pop_ms.append((time.perf_counter() - t0) * 1e3)
    after = list(g.counts())
    g.close()
print(json.dumps({"reads": n, "genome": G, "err": err, "k": k, "good_kmers": good, "graph": [nodes, edges, length],
                  "candidate_edges": int(len(cand_ids)), "candidate_share": round(len(cand_ids) / max(edges, 1), 6), "pairs_compared": pairs,
                  "bubbles_removed": removed, "tips_removed": tips, "pop_bubbles_ms": [round(x, 3) for x in pop_ms], "clip_tips_ms": [round(x, 3) for x in clip_ms],
                  "edge_distance_ms": [round(x, 3) for x in dist_ms], "edge_distance_pairs": int(same.sum()), "within_3": int((dist <= 3).sum()),
                  "pop_over_clip": round(min(pop_ms) / min(clip_ms), 3), "graph_after_pop": after}))
m.close(); ctx.free(d); ctx.close()
