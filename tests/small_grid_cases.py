"""Inputs of tests/test_small_grid_gpu.py, sized on the CPU oracle so that a launch grid of 1 or 3 workgroups ("test_max_grid")
makes every workgroup take at least two trips through its grid-stride loop, the last with a partly filled wave.  What the
graphs ARE is for the oracle and the restatements to say: nothing here is an expected value, and every size the test relies
on is asserted there from the reference side.

reads_case(k)        reads over a two-haplotype genome, k-mers seen once dropped: the graph of build -> retain
planted_case(k)      a k-mer set with counts (add_counts): FRAGMENTS isolated pieces of k + 2 bases — each a two-node component
                     per strand, far more components than one workgroup's LDS table holds — beside GENOMES planted genomes of
                     one plan (SNP bubbles, dead-end arms; tests/bubbles_planted.py), hence of one node count: the components
                     tied for largest, two per genome.  The first genome has long edges between its elements, the others
                     short ones of a length of their own, so that no two components agree in (nodes, length) by construction.
"""
import random

from oracle import pyref as R

import bubbles_planted as P

# gk_tile.h: threads per workgroup of every grid-stride kernel; gk_scan.h: elements per workgroup of scan_counts; gk_graph_ops.hip:
# entries of a workgroup's LDS component table (CcTable) — a root that finds 16 probed entries taken goes straight to memory
BLOCK = 256
SCAN_CHUNK = 4096
CC_TAB = 1024

# k -> (reads, read length, genome length, bases between the second haplotype's SNPs): the smallest of the sizes tried at which
# the oracle's graph has more than 2 * 3 * BLOCK nodes and edges, neither a multiple of 64 (asserted by the test).  The SNPs are
# further apart than k where k is large, so that every one of them is a clean bubble of four nodes and six edges.
READS = {11: (1600, 60, 6000, 17), 35: (4000, 100, 20000, 57), 64: (3840, 150, 24000, 86)}


def reads_case(k):
    n, ln, glen, step = READS[k]
    rnd = random.Random(1000 + k)
    g = "".join(rnd.choice("AGCT") for _ in range(glen))
    h = list(g)
    for p in range(30, glen, step):
        h[p] = rnd.choice([c for c in "AGCT" if c != h[p]])
    haps = [g, "".join(h)]
    out = []
    for _ in range(n):
        hp = rnd.choice(haps)
        s = rnd.randrange(0, glen - ln + 1)
        r = hp[s:s + ln]
        if rnd.random() < 0.5:
            r = R.rev_comp(r)
        out.append("".join(c if rnd.random() >= 0.01 else rnd.choice([x for x in "AGCT" if x != c]) for c in r))
    return out


FRAGMENTS = {31: 1103, 34: 1103}
GENOMES = 9
C_FRAGMENT = 4


def _plan(spacer):
    snp = ("bubble", 1, ("subs", 1), 3)
    return [(snp, spacer), (("arms", [None], 2), spacer), (("bubble", 6, ("subs", 3), 3), spacer), (snp, spacer),
            (("arms", [None, ("sub_last",)], 2), spacer), (("bubble", 9, ("ins", 3, 2), 4), spacer)]


def planted_case(k):
    """-> counts (stored k-mer -> count)"""
    rnd = random.Random(77 * k)
    counts = {}
    for _ in range(FRAGMENTS[k]):
        P.add_piece(counts, "".join(rnd.choice("AGCT") for _ in range(k + 2)), C_FRAGMENT, k)
    for i in range(GENOMES):
        _g, c = P.planted(k, _plan(180 if i == 0 else 4 + i), seed=500 * k + i)
        for key, v in c.items():
            counts[key] = counts.get(key, 0) + v
    return counts
