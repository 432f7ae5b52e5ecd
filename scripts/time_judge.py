"""What the placement pass and the judge cost: time_overlap_gaps.py's set-up (a 4 Mbp genome by default, 30x of 150 bp mates = 4e5
pairs, inserts 230..300, 0.5 % error, k = 31), count -> filter -> buildGraph -> retain -> getGraphMap -> pairLinks -> joins ->
chains -> scaffold plan, then REPS times each: gk_placements_add_record over the genome as one reference record (wall ms of
create + add + stats, and the lookup kernel's device ms), gk_scaffolds_judge on the plan (wall ms), and gk_fasta_check over the same
genome as FASTA text (wall ms and its lookup kernels' device ms): the check makes ONE `contains` lookup per window, the placement
pass TWO getAll lookups and the fold.  tol = half the width of the insert range (a choice).
    python scripts/time_judge.py [genome bases] [tol]
(profiles/r16/judge_*.txt)"""
import sys, time, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from genome_amd import _lib as L
from genome_amd.check import FastaCheck, scaffold_n50s
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
record = np.frombuffer(b"AGCT", np.uint8)[genome].tobytes()
fasta = b">genome\n" + record + b"\n"
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
plan = g.scaffolds(chains, gaps, line_width=WIDTH)
print(f"linked {cls['linked']}, joins {jst['joins']}, chains {len(chains)} of {sum(len(c) for c in chains)} members, plan {plan.stats()['records']} records")
ms = {"place_wall": [], "place_kernel": [], "judge_wall": [], "fasta_check_wall": [], "fasta_check_lookup": []}
for rep in range(REPS + 1):                          # (the first round warms the block pool and the kernels' code up)
    t0 = time.perf_counter()
    pl = g.place(vm, [record])
    pst = pl.stats()
    t_place = (time.perf_counter() - t0) * 1e3
    t_kernel = pl.last_ms()["lookup_kernels"]
    t0 = time.perf_counter()
    res = plan.judge(pl, TOL)
    t_judge = (time.perf_counter() - t0) * 1e3
    pl.close()
    t0 = time.perf_counter()
    with FastaCheck(ctx, vm) as fc:
        fc.feed(fasta, last=True)
        cst, t_look = fc.stats(), fc.last_ms()["lookup"]
    t_check = (time.perf_counter() - t0) * 1e3
    if rep:
        for name, v in zip(ms, (t_place, t_kernel, t_judge, t_check, t_look)):
            ms[name].append(v)
med = lambda v: float(np.median(v))
for name, v in ms.items():
    print("%s ms: median %.3f, min %.3f, max %.3f over %d calls" % (name, med(v), min(v), max(v), REPS))
print("place_kernel / fasta_check_lookup: %.2f   (%.3f ns per window for the two getAll lookups and the fold, %.3f ns for the one contains and the cover pass)" % (
    med(ms["place_kernel"]) / med(ms["fasta_check_lookup"]), med(ms["place_kernel"]) * 1e6 / pst["windows"], med(ms["fasta_check_lookup"]) * 1e6 / cst["windows"]))
print("placements:", pst)
print("fasta check: windows %d, found %d" % (cst["windows"], cst["found"]))
print("judge, tol %d:" % TOL, {n: v for n, v in res["stats"].items() if v})
print("n50:", scaffold_n50s(plan.segments(), res["classes"]))
# which edges the genome's forward strand leaves unplaced: the same pass over the reverse complement of the genome
ne = g.idBounds()[1]
info = g.edgesById(np.arange(ne, dtype=np.uint32))
rc_record = np.frombuffer(b"TCGA", np.uint8)[genome[::-1]].tobytes()
with g.place(vm, [record]) as a, g.place(vm, [rc_record]) as b:
    ca, cb = a.edges()["cls"], b.edges()["cls"]
un = [e for e in range(ne) if info["alive"][e] and ca[e] == "unplaced"]
print("unplaced on the forward strand: %d; of them placed by the reverse complement of the genome: %d, with len == 1: %d, neither: %d" % (
    len(un), sum(cb[e] in ("forward", "reverse") for e in un), sum(int(info["len"][e]) == 1 for e in un),
    sum(cb[e] not in ("forward", "reverse") and int(info["len"][e]) != 1 for e in un)))
