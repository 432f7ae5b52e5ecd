"""What overlap detection costs beside the scaffold plan: time_fill_gaps.py's set-up (a 4 Mbp genome by default, 30x of 150 bp mates
= 4e5 pairs, inserts 230..300, 0.5 % error, k = 31), count -> filter -> buildGraph -> retain -> getGraphMap -> pairLinks -> joins ->
chains, then REPS times each: gk_graph_overlap_gaps on those chains (tol = half the width of the insert range, min_overlap 10,
max_overlap k: the defaults, which are choices) and gk_graph_scaffolds_plan on the same chains, and once the plan with the
overlaps, for the N bases that went.  Wall time of the whole call, the host's flattening of the lists included.
    python scripts/time_overlap_gaps.py [genome bases] [tol]
(profiles/r14/overlap_gaps_*.txt)"""
import sys, time, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from genome_amd import _lib as L
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.graph import HipLinks, buildGraph, scaffoldChains, scaffoldGaps

G, L_, k, cov, err = int(sys.argv[1]) if len(sys.argv) > 1 else 4_000_000, 150, 31, 30, 0.005
MAX_SPAN, MID, WIDTH, TOL = 300 + k, 265, 60, int(sys.argv[2]) if len(sys.argv) > 2 else 35
REPS = 7
rng = np.random.default_rng(7)
genome = rng.integers(0, 4, G, dtype=np.uint8)
npairs = 4_000_000 * cov // (2 * L_) if G < 4_000_000 else G * cov // (2 * L_)
ins = rng.integers(230, 301, npairs)
start = rng.integers(0, G - 300, npairs)
flip = rng.random(npairs) < 0.5
comp = np.array([3, 2, 1, 0], np.uint8)            # A0 G1 C2 T3: complement = 3 - b
reads = np.empty((2 * npairs, L_), np.uint8)
idx = np.arange(L_)
for i in range(0, npairs, 100000):
    j = min(npairs, i + 100000)
    a = genome[start[i:j, None] + idx[None, :]]
    b = comp[genome[(start[i:j] + ins[i:j])[:, None] - 1 - idx[None, :]]]
    f = flip[i:j, None]
    reads[2 * i:2 * j:2] = np.where(f, b, a)
    reads[2 * i + 1:2 * j:2] = np.where(f, a, b)
e = rng.random(reads.shape) < err
reads = np.where(e, (reads + rng.integers(1, 4, reads.shape, dtype=np.uint8)) & 3, reads).astype(np.uint8)
pad = np.zeros((2 * npairs, 152), np.uint8); pad[:, :L_] = reads
packed = (pad[:, 0::4] | (pad[:, 1::4] << 2) | (pad[:, 2::4] << 4) | (pad[:, 3::4] << 6)).astype(np.uint8)
binb = np.concatenate([np.full((2 * npairs, 1), L_, np.uint8), packed], axis=1).tobytes()
ctx = Context(0)
m = HipDNAMap(ctx, k)
m.count_reads(binb, 2 * npairs); m.deleteAll_lt(3)
g = buildGraph(k, m); g.retainLargest()
vm = g.getGraphMap()
print(f"library {os.path.basename(L.LIB_PATH)}: genome {G}, {npairs} pairs, k {k}, graph {g.counts()}, {vm.size()} positions, max_span {MAX_SPAN}")
links = HipLinks(ctx)
cls = g.pairLinks(vm, (binb, npairs), links, min_len=2 * k, max_span=MAX_SPAN)
joins, jst = links.joins(3)
chains = scaffoldChains(joins[0], joins[1])
gaps = scaffoldGaps(chains, joins, MID)
print(f"linked {cls['linked']}, joins {jst['joins']}, chains {len(chains)} of {sum(len(c) for c in chains)} members, line width {WIDTH}")
ms = {"overlap_gaps": [], "scaffold_plan": []}
for rep in range(REPS + 1):                          # (the first round warms the block pool and the kernels' code up)
    t0 = time.perf_counter()
    ov, rep_ = g.overlapGaps(chains, gaps, TOL)
    t_ovl = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    p = g.scaffolds(chains, gaps, line_width=WIDTH)
    t_plan = (time.perf_counter() - t0) * 1e3
    plain = p.stats()
    p.close()
    if rep:
        ms["overlap_gaps"].append(t_ovl); ms["scaffold_plan"].append(t_plan)
p = g.scaffolds(chains, gaps, line_width=WIDTH, overlaps=ov)
joined, ost = p.stats(), p.overlapStats()
p.close()
med = lambda v: float(np.median(v))
for name, v in ms.items():
    print("%s ms: median %.3f, min %.3f, max %.3f over %d calls" % (name, med(v), min(v), max(v), REPS))
print("overlap_gaps / scaffold_plan: %.2f" % (med(ms["overlap_gaps"]) / med(ms["scaffold_plan"])))
print("tol %d, min_overlap 10, max_overlap %d: %s" % (TOL, k, {n: v for n, v in rep_.items() if n != "classes"}))
print("N bases %d -> %d, gapped junctions %d -> %d, clamped %d -> %d, overlapped %d dropping %d bases" % (
    plain["n_bases"], joined["n_bases"], plain["gapped"], joined["gapped"], plain["clamped"], joined["clamped"], ost["overlapped"], ost["dropped"]))
