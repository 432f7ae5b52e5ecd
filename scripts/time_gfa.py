"""What the twin pass and the GFA text cost beside the contig FASTA of the same graph: time_thread_spans.py's set-up (a 4 Mbp genome
by default, 30x of 150 bp mates = 4e5 pairs, 0.5 % error, k = 31), count -> filter -> buildGraph, and the graph is taken as built,
before any simplification: the largest edge count.  Then REPS times, alternating in one run: gk_graph_edge_twins (no ids asked:
the six stats alone), gk_graph_gfa_plan + gk_gfa_write, and gk_graph_contigs_plan(strands = 1) + gk_contigs_write — unchanged
code that emits the same bases, the yardstick.  Wall ms, medians, the two byte counts; the result also goes to OUT if given.
    python scripts/time_gfa.py [genome bases] [pairs] [OUT]
The library under GK_LIB_PATH is the one timed."""
import sys, time, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from genome_amd import _lib as L
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.graph import buildGraph

G, L_, k, cov, err = int(sys.argv[1]) if len(sys.argv) > 1 else 4_000_000, 150, 31, 30, 0.005
npairs = int(sys.argv[2]) if len(sys.argv) > 2 else G * cov // (2 * L_)
OUT = sys.argv[3] if len(sys.argv) > 3 else None
DIR = "/dev/shm" if os.path.isdir("/dev/shm") else "."
REPS = 5
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
ctx = Context(0)
m = HipDNAMap(ctx, k)
m.count_reads(rec.tobytes(), 2 * npairs); m.deleteAll_lt(3)
g = buildGraph(k, m)
lines = [f"library {os.path.basename(L.LIB_PATH)}: genome {G}, {npairs} pairs, k {k}, graph as built {g.counts()}"]
none = np.zeros(0, np.uint32)
med = lambda v: float(np.median(v))
twins_ms, gfa_ms, contigs_ms = [], [], []
gfa_path, fa_path = os.path.join(DIR, "time_gfa.gfa"), os.path.join(DIR, "time_gfa.fa")
for rep in range(REPS + 1):                          # (the first round warms the block pool and the kernels' code up)
    t0 = time.perf_counter(); _, _, tst = g.edgeTwins(none); t = (time.perf_counter() - t0) * 1e3
    if rep:
        twins_ms.append(t)
    t0 = time.perf_counter(); p = g.gfa(); p.write(gfa_path); t = (time.perf_counter() - t0) * 1e3
    gst, gemit = p.stats(), p.last_ms()["emit_kernels"]
    p.close()
    if rep:
        gfa_ms.append(t)
    t0 = time.perf_counter(); c = g.contigs(line_width=0, strands=1); c.write(fa_path); t = (time.perf_counter() - t0) * 1e3
    cst, cemit = c.stats(), c.last_ms()["emit_kernels"]
    c.close()
    if rep:
        contigs_ms.append(t)
for p in (gfa_path, fa_path):
    os.unlink(p)
lines += [f"twins {tst}",
          f"gfa {gst}",
          f"gk_graph_edge_twins                         {med(twins_ms):9.3f} ms   (median of {REPS})",
          f"gk_graph_gfa_plan + gk_gfa_write            {med(gfa_ms):9.3f} ms   {gst['text_bytes']} bytes   (emit kernels of the last write {gemit:.3f} ms)",
          f"gk_graph_contigs_plan(1) + gk_contigs_write {med(contigs_ms):9.3f} ms   {cst['text_bytes']} bytes   (emit kernels of the last write {cemit:.3f} ms)",
          f"gfa / contigs                               {med(gfa_ms) / med(contigs_ms):9.2f} x"]
print("\n".join(lines))
if OUT:
    with open(OUT, "w") as fh:
        fh.write("\n".join(lines) + "\n")
g.close(); m.close(); ctx.close()
