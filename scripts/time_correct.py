"""gk_reads_correct_dev on reads resident in HBM (mode-G synthetic reads with substitution errors, 150 bases, k = 31), beside two
numbers from the same run: gk_map_count_reads_dev of the same reads (the insert), and gk_graph_edge_coverage's lookup rate on the
graph built from them after deleteAll(< solid) (the other reader of the count table).  solid = the valley of the count's spectrum.
Lookups of the correction = windows + 3 x the weak windows of accepted runs, counted as corrected/ambiguous/unresolved runs x k
at most: the JSON reports windows and the bound separately.
usage: python scripts/time_correct.py [reads=1000000] [genome=4600000] [err=0.005] [k=31] [reps=3] [out.json]
Prints one JSON line (and writes it to out.json when given)."""
import sys, time, json, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from genome_amd import synth
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.graph import buildGraph

arg = lambda i, d, f=int: f(sys.argv[i]) if len(sys.argv) > i else d
n, G, err, k, reps = arg(1, 1_000_000), arg(2, 4_600_000), arg(3, 0.005, float), arg(4, 31), arg(5, 3)
out_path = arg(6, "", str)
L = 150
ctx = Context(0)
nbytes = n * synth.record_stride(L)
d, d_out = ctx.alloc(nbytes + 64), ctx.alloc(nbytes + 64)
ctx.synth_reads(d, n, L, "G", 3, 0, G, err)
count_ms = []
for _ in range(reps):
    m = HipDNAMap(ctx, k, 0)
    ctx.sync()
    t0 = time.perf_counter(); occ = m.count_reads_dev(d, n, L); count_ms.append((time.perf_counter() - t0) * 1e3)
    if _ + 1 < reps:
        m.close()
info = m._solid("auto")
solid = info["solid"]
cor_ms = []
for _ in range(reps):
    ctx.sync()
    t0 = time.perf_counter(); st = m.correct_reads_dev(d, n, L, solid, d_out); cor_ms.append((time.perf_counter() - t0) * 1e3)
judged = st["corrected"] + st["ambiguous"] + st["unresolved"]
lookups_min, lookups_max = st["windows"], st["windows"] + 3 * k * judged
# the other reader of the table: edge coverage on the graph of the same reads
m.deleteAll_lt(solid)
g = buildGraph(k, m)
ids = np.arange(g.idBounds()[1], dtype=np.uint32)
cov_ms = []
for _ in range(reps):
    ctx.sync()
    t0 = time.perf_counter(); c = g.edgeCoverage(m, ids); cov_ms.append((time.perf_counter() - t0) * 1e3)
probes = int(c["kmers"].sum())
res = {"reads": n, "read_len": L, "genome": G, "err": err, "k": k, "solid": solid, "solid_auto": info.get("solid_auto"), "stats": {a: st[a] for a in st if a not in info},
       "correct_ms": [round(x, 3) for x in cor_ms], "lookups_at_least": lookups_min, "lookups_at_most": lookups_max,
       "correct_lookups_per_s": [round(lookups_min / (min(cor_ms) * 1e-3), 1), round(lookups_max / (min(cor_ms) * 1e-3), 1)],
       "count_reads_dev_ms": [round(x, 3) for x in count_ms], "count_windows_per_s": round(occ / (min(count_ms) * 1e-3), 1),
       "edge_coverage_ms": [round(x, 3) for x in cov_ms], "edge_coverage_probes": probes, "edge_coverage_probes_per_s": round(probes / (min(cov_ms) * 1e-3), 1)}
line = json.dumps(res)
print(line)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").write(line + "\n")
g.close(); m.close(); ctx.free(d); ctx.free(d_out); ctx.close()
