"""What following the reads across whole edges costs beside threading them through single nodes: time_thread_reads.py's set-up
(a 4 Mbp genome by default, 30x of 150 bp mates = 4e5 pairs, 0.5 % error, k = 31), count -> filter -> buildGraph -> retain ->
getGraphMap, the records uploaded once, then REPS times, alternating in one run: gk_graph_thread_reads_dev (the yardstick: the
same two position-map probes per window) and gk_graph_thread_spans_dev (the same probes plus LDS work).  Wall ms, medians, and
the ratio.  Then, once, how many edges gk_graph_split_edges_by_spans finds to be candidates and how many it resolves at CUTOFF
(default 3: a choice, not a measurement).  A small genome (2000) is the hot case: every read crosses the same few nodes.
    python scripts/time_thread_spans.py [genome bases] [pairs] [cutoff]
The library under GK_LIB_PATH is the one timed."""
import sys, time, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from genome_amd import _lib as L
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.graph import HipSpans, Support, buildGraph

G, L_, k, cov, err = int(sys.argv[1]) if len(sys.argv) > 1 else 4_000_000, 150, 31, 30, 0.005
npairs = int(sys.argv[2]) if len(sys.argv) > 2 else G * cov // (2 * L_)
CUTOFF = int(sys.argv[3]) if len(sys.argv) > 3 else 3
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
m.count_reads(binb, nreads); m.deleteAll_lt(3)
g = buildGraph(k, m); g.retainLargest()
vm = g.getGraphMap()
d = ctx.alloc(rec.size + 64)
ctx.upload(d, rec)
windows = nreads * (L_ - k + 1)
print(f"library {os.path.basename(L.LIB_PATH)}: genome {G}, {npairs} pairs, k {k}, graph {g.counts()}, {vm.size()} positions, {windows} windows")
med = lambda v: float(np.median(v))
reads_ms, spans_ms = [], []
for rep in range(REPS + 1):                          # (the first round warms the block pool and the kernels' code up)
    sup = Support(ctx)
    t0 = time.perf_counter(); st7 = g.threadReadsDev(vm, sup, d, nreads, L_); t = (time.perf_counter() - t0) * 1e3
    if rep:
        reads_ms.append(t)
    sup.close()
    sp = HipSpans(ctx)
    t0 = time.perf_counter(); st5 = g.threadSpansDev(vm, sp, d, nreads, L_); t = (time.perf_counter() - t0) * 1e3
    if rep:
        spans_ms.append(t)
    if rep < REPS:
        sp.close()
assert st5["crossings"] == st7["crossings"]
print("thread stats:", st7)
print("span stats:", st5, " distinct (e, m, f):", sp.size()[0])
for name, v in (("thread_reads_dev", reads_ms), ("thread_spans_dev", spans_ms)):
    print("%s ms: median %.3f, min %.3f, max %.3f over %d calls; %.3g windows/s" % (name, med(v), min(v), max(v), REPS, windows / med(v) * 1e3))
print("thread_spans / thread_reads = %.2f" % (med(spans_ms) / med(reads_ms)))
t0 = time.perf_counter(); est = g.splitEdgesBySpans(sp, CUTOFF); t = (time.perf_counter() - t0) * 1e3
print("split_edges_by_spans at cutoff %d: %s in %.3f ms" % (CUTOFF, est, t))
