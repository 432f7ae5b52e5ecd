"""What the alignment-block pass costs beside the placement pass it doubles: time_judge.py's set-up (a 4 Mbp genome by default, 30x
of 150 bp mates = 4e5 pairs, inserts 230..300, 0.5 % error, k = 31), count -> filter -> buildGraph -> retain -> getGraphMap, then
REPS times, alternating in one run: gk_placements_add_record over the genome as one reference record (wall ms of create + add +
stats, and k_place_windows' device ms: the yardstick, code this pass does not touch), and gk_blocks_add_record + gk_blocks_finish
over the same record (wall ms of create + add + finish + stats; the count launches with their scans, the emit launches and the
finish's device ms).  The pass looks every window up twice, so count + emit against k_place_windows is the measured price of that.
Then what the blocks say about the edges, class by class against the placements' classes.  tol defaults to 1000 (a choice).
    python scripts/time_blocks.py [genome bases] [tol]
(profiles/r17/blocks_*.txt)"""
import sys, time, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from collections import Counter
import numpy as np
from genome_amd import _lib as L
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.graph import buildGraph

G, L_, k, cov, err = int(sys.argv[1]) if len(sys.argv) > 1 else 4_000_000, 150, 31, 30, 0.005
TOL = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
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
record = np.frombuffer(b"AGCT", np.uint8)[genome].tobytes()
ctx = Context(0)
m = HipDNAMap(ctx, k)
m.count_reads(binb, 2 * npairs); m.deleteAll_lt(3)
g = buildGraph(k, m); g.retainLargest()
vm = g.getGraphMap()
print(f"library {os.path.basename(L.LIB_PATH)}: genome {G}, {npairs} pairs, k {k}, graph {g.counts()}, {vm.size()} positions")
names = ("place_wall", "place_kernel", "blocks_wall", "blocks_count", "blocks_emit", "blocks_finish_kernels", "blocks_finish_wall")
ms = {n: [] for n in names}
for rep in range(REPS + 1):                          # (the first round warms the block pool and the kernels' code up)
    t0 = time.perf_counter()
    pl = g.place(vm, [record])
    pst = pl.stats()
    t_place = (time.perf_counter() - t0) * 1e3
    t_kernel = pl.last_ms()["lookup_kernels"]
    pl.close()
    t0 = time.perf_counter()
    bl = g.alignBlocks(vm, [record], TOL)
    bst = bl.stats()
    t_blocks = (time.perf_counter() - t0) * 1e3
    lm = bl.last_ms()
    bl.close()
    if rep:
        for name, v in zip(names, (t_place, t_kernel, t_blocks, lm["count_kernels"], lm["emit_kernels"], lm["finish_kernels"], lm["finish_total"])):
            ms[name].append(v)
med = lambda v: float(np.median(v))
for name, v in ms.items():
    print("%s ms: median %.3f, min %.3f, max %.3f over %d calls" % (name, med(v), min(v), max(v), REPS))
print("(blocks_count + blocks_emit) / place_kernel: %.2f   (blocks_count alone: %.2f; %.3f ns per window for the four lookups, %.3f ns for the placements' two)" % (
    (med(ms["blocks_count"]) + med(ms["blocks_emit"])) / med(ms["place_kernel"]), med(ms["blocks_count"]) / med(ms["place_kernel"]),
    (med(ms["blocks_count"]) + med(ms["blocks_emit"])) * 1e6 / bst["windows"], med(ms["place_kernel"]) * 1e6 / pst["windows"]))
print("placements:", pst)
print("blocks, tol %d:" % TOL, bst)
# what the blocks say about the edges, against the placements' classes
with g.place(vm, [record]) as pl, g.alignBlocks(vm, [record], TOL) as bl:
    pc, be = pl.edges()["cls"], bl.edges()
    n = bl.na50()
    info = g.edgesById(np.arange(g.idBounds()[1], dtype=np.uint32))
    live = [e for e in range(len(pc)) if info["alive"][e]]
    print("edges by (placement class, block class, full):", sorted(Counter((pc[e], be["cls"][e], be["full"][e]) for e in live).items()))
    print("genome fraction %.6f, NA50 %d, NGA50 %d, pieces %d of %d bases" % (bst["covered"] / max(bst["windows"], 1), n["na50"], n["nga50"], bst["pieces"], bst["piece_bases"]))
