"""What the insert-range estimate costs beside the walks it precedes: time_walk_pairs.py's library (a 4 Mbp genome by default,
30x of 150 bp mates = 4e5 pairs, inserts 230..300, 0.5 % error, k = 31), count -> filter -> buildGraph -> retain -> getGraphMap,
then REPS times each: walkPairs (its phases: keys, the getAll batch, checks, walks) and pairDistances (wall; the two calls share
the front end, so pairDistances minus walkPairs' keys + lookup is the position check, k_pair_distances and the read-back).
Kernel times come from running this script under `rocprofv3 --kernel-trace --stats`: k_pair_distances against k_vm_get_all.
    python scripts/time_pair_distances.py [genome bases] [bins]
The library under GK_LIB_PATH (any build that has gk_graph_walk_pairs) is the one timed: a build without
gk_graph_pair_distances times walkPairs alone (the before / after of the front end's refactor)."""
import sys, time, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes as C
import numpy as np
from genome_amd import _lib as L

if not hasattr(C.CDLL(L.LIB_PATH), "gk_graph_pair_distances"):          # an older build: bind what it has
    for name in ("gk_graph_pair_distances", "gk_insert_range", "gk_dist_pair_distances"):
        L.SIGNATURES.pop(name)
    HAVE = False
else:
    HAVE = True
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.graph import Support, buildGraph, insertRange

G, L_, k, cov, err = int(sys.argv[1]) if len(sys.argv) > 1 else 4_000_000, 150, 31, 30, 0.005
BINS = int(sys.argv[2]) if len(sys.argv) > 2 else 512
REPS = 7
rng = np.random.default_rng(7)
genome = rng.integers(0, 4, G, dtype=np.uint8)
npairs = G * cov // (2 * L_)
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
print(f"library {os.path.basename(L.LIB_PATH)}: genome {G}, {npairs} pairs, k {k}, graph {g.counts()}, {vm.size()} positions, bins {BINS}")
walk_ms, phases, dist_ms = [], [], []
for rep in range(REPS + 1):                          # (the first round warms the block pool and the kernels' code up)
    sup = Support(ctx)
    t0 = time.perf_counter(); g.walkPairs(vm, sup, binb, npairs, 180, 250); t = (time.perf_counter() - t0) * 1e3
    if rep:
        walk_ms.append(t); phases.append(sup.last_ms())
    walked = sup.sizes()
    sup.close()
    if HAVE:
        t0 = time.perf_counter(); hist, classes = g.pairDistances(vm, (binb, npairs), bins=BINS); t = (time.perf_counter() - t0) * 1e3
        if rep:
            dist_ms.append(t)
med = lambda v: float(np.median(v))
print("walkPairs ms: median %.3f, min %.3f, max %.3f over %d calls; (pairs, bad, walked) = %s" % (med(walk_ms), min(walk_ms), max(walk_ms), REPS, walked))
print("walkPairs phases ms (medians):", {key: round(med([p[key] for p in phases]), 3) for key in phases[0]})
if HAVE:
    front = med([p["keys"] + p["lookup"] for p in phases])
    print("pairDistances ms: median %.3f, min %.3f, max %.3f; minus the shared front end (keys + lookup, %.3f): %.3f for check + k_pair_distances + read-back"
          % (med(dist_ms), min(dist_ms), max(dist_ms), front, med(dist_ms) - front))
    print("classes:", classes)
    print("insert range (trim 25, min 1000):", insertRange(hist), " occupied bins:", int((hist > 0).sum()))
