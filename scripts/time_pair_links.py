"""What the scaffold links cost beside the insert-range estimate: time_pair_distances.py's library (a 4 Mbp genome by default, 30x
of 150 bp mates = 4e5 pairs, inserts 230..300, 0.5 % error, k = 31), count -> filter -> buildGraph -> retain -> getGraphMap,
then REPS times each: pairDistances and pairLinks into a fresh table.  The two share the front end (keys, the getAll batch, the
position check), so their difference is k_pair_distances against k_pair_links + the table's reserve and merge.  Then joins.
    python scripts/time_pair_links.py [genome bases] [max_span]
(profiles/r11/pair_links_*.txt; the in-wave combine those files also time was removed after it did not win.)"""
import sys, time, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from genome_amd import _lib as L
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.graph import HipLinks, buildGraph

G, L_, k, cov, err = int(sys.argv[1]) if len(sys.argv) > 1 else 4_000_000, 150, 31, 30, 0.005
MAX_SPAN = int(sys.argv[2]) if len(sys.argv) > 2 else 300 + k
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
forms = [("plain", -1)]
dist_ms, link_ms, joins_ms = [], {name: [] for name, _ in forms}, []
for rep in range(REPS + 1):                          # (the first round warms the block pool and the kernels' code up)
    t0 = time.perf_counter(); hist, dcls = g.pairDistances(vm, (binb, npairs), bins=512); t = (time.perf_counter() - t0) * 1e3
    if rep:
        dist_ms.append(t)
    for name, v in forms:
        links = HipLinks(ctx)
        t0 = time.perf_counter(); cls = g.pairLinks(vm, (binb, npairs), links, min_len=2 * k, max_span=MAX_SPAN); t = (time.perf_counter() - t0) * 1e3
        if rep:
            link_ms[name].append(t)
        if name == "plain":
            size = links.size()
            t0 = time.perf_counter(); joins, st = links.joins(3); t = (time.perf_counter() - t0) * 1e3
            if rep:
                joins_ms.append(t)
        links.close()
med = lambda v: float(np.median(v))
print("pairDistances ms: median %.3f, min %.3f, max %.3f over %d calls" % (med(dist_ms), min(dist_ms), max(dist_ms), REPS))
for name, _ in forms:
    v = link_ms[name]
    print("pairLinks (%s) ms: median %.3f, min %.3f, max %.3f; / pairDistances = %.3f" % (name, med(v), min(v), max(v), med(v) / med(dist_ms)))
print("joins(3) ms: median %.3f; stats %s" % (med(joins_ms), st))
print("classes:", cls, " (links, observations):", size, " apart in pairDistances:", dcls["apart"])
