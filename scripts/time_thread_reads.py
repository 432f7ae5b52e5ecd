"""What threading the reads through the graph costs beside a count of the same reads and the pair walk of the same pairs:
time_pair_distances.py's library (a 4 Mbp genome by default, 30x of 150 bp mates = 4e5 pairs, inserts 230..300, 0.5 % error,
k = 31), count -> filter -> buildGraph -> retain -> getGraphMap, the records uploaded once, then REPS times each:
gk_graph_thread_reads_dev (wall ms, windows/s over both strands' lookups = 2 per window), the same call with the in-wave combine
on (the test build's "thread_combine" = 1), gk_map_count_reads_dev of the same records into a fresh table (one table line per
window where threading touches two: the yardstick, the count table being a different table), and gk_graph_walk_pairs of the
same pairs.  A small genome (2000) is the hot-counter case: every read crosses the same few nodes.
    python scripts/time_thread_reads.py [genome bases] [pairs] [nowalk]
The library under GK_LIB_PATH is the one timed; the A/B needs the test build (the product library has no switches).  nowalk: the
pair walk is left out (on the small genome its graph of error k-mers makes every walk long)."""
import sys, time, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from genome_amd import _lib as L
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.graph import Support, buildGraph

G, L_, k, cov, err = int(sys.argv[1]) if len(sys.argv) > 1 else 4_000_000, 150, 31, 30, 0.005
npairs = int(sys.argv[2]) if len(sys.argv) > 2 else G * cov // (2 * L_)
WALK = not (len(sys.argv) > 3 and sys.argv[3] == "nowalk")
REPS = 7
rng = np.random.default_rng(7)
genome = rng.integers(0, 4, G, dtype=np.uint8)
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
rec = np.ascontiguousarray(np.concatenate([np.full((2 * npairs, 1), L_, np.uint8), packed], axis=1))
binb, nreads = rec.tobytes(), 2 * npairs
ctx = Context(0)
m = HipDNAMap(ctx, k)
occ = m.count_reads(binb, nreads); m.deleteAll_lt(3)
g = buildGraph(k, m); g.retainLargest()
vm = g.getGraphMap()
d = ctx.alloc(rec.size + 64)
ctx.upload(d, rec)
windows = nreads * (L_ - k + 1)
print(f"library {os.path.basename(L.LIB_PATH)}: genome {G}, {npairs} pairs, k {k}, graph {g.counts()}, {vm.size()} positions, {windows} windows")
try:
    ctx.set_option("thread_combine", -1)
    forms = (("no combine", -1), ("combine", 1))
except (L.GkError, AttributeError):                 # the product library has no switches: the default form only
    forms = (("no combine", None),)
med = lambda v: float(np.median(v))
ms = {name: [] for name, _ in forms}
count_ms, walk_ms = [], []
for rep in range(REPS + 1):                          # (the first round warms the block pool and the kernels' code up)
    for name, v in forms:
        if v is not None:
            ctx.set_option("thread_combine", v)
        sup = Support(ctx)
        t0 = time.perf_counter(); st = g.threadReadsDev(vm, sup, d, nreads, L_); t = (time.perf_counter() - t0) * 1e3
        if rep:
            ms[name].append(t)
        pairs = sup.sizes()[0]
        sup.close()
    if forms[0][1] is not None:
        ctx.set_option("thread_combine", -1)
    c = HipDNAMap(ctx, k, occ)
    t0 = time.perf_counter(); c.count_reads_dev(d, nreads, L_); t = (time.perf_counter() - t0) * 1e3
    if rep:
        count_ms.append(t)
    c.close()
    if WALK:
        sup = Support(ctx)
        t0 = time.perf_counter(); g.walkPairs(vm, sup, binb, npairs, 180, 250); t = (time.perf_counter() - t0) * 1e3
        if rep:
            walk_ms.append(t)
        sup.close()
print("stats:", st, " distinct (in, out) pairs:", pairs)
for name, _ in forms:
    v = ms[name]
    print("thread_reads_dev (%s) ms: median %.3f, min %.3f, max %.3f over %d calls; %.3g windows/s, %.3g lookups/s"
          % (name, med(v), min(v), max(v), REPS, windows / med(v) * 1e3, 2 * windows / med(v) * 1e3))
print("count_reads_dev ms: median %.3f, min %.3f, max %.3f; %.3g windows/s; thread / count = %.2f"
      % (med(count_ms), min(count_ms), max(count_ms), windows / med(count_ms) * 1e3, med(ms[forms[0][0]]) / med(count_ms)))
if WALK:
    print("walkPairs ms: median %.3f, min %.3f, max %.3f; thread / walk = %.2f" % (med(walk_ms), min(walk_ms), max(walk_ms), med(ms[forms[0][0]]) / med(walk_ms)))
