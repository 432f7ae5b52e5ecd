"""Hand-written graphs for the bubble rule (tests/test_bubbles_cpu.py holds the restatement to them, tests/test_bubbles_gpu.py
the device), in the style of tests/tips_cases.py and on its genome.

Each case is the genome G (count 10) plus, at a lower count, second copies of a middle stretch that carry a variant: the W bases
G[J:J+W] replaced by V.  A copy is the piece G[J-K+1:J] ++ V ++ G[J+W:J+W+K-1] — every window that holds a base of V, none of
the genome's own — so the graph is

    G[:J]  ->  the branch node G[J-K:J]  =>  one edge per variant, and the genome's own  =>  the merge node G[J+W:J+W+K]  ->  G[J+W:]

The genome's branch spells G[J:J+W+K]: W + K bases, W + K + 1 windows, all at count 10.  A variant's spells V ++ G[J+W:J+W+K]:
|V| + K bases; of its |V| + K + 1 windows the first and the last are the two nodes (count 10) and the |V| + K - 1 between them
are the copy's.  V differs from G[J:J+W] in its first base (out-edges of one node differ there) and from the base before the
merge node (G[J+W-1], or G[J-1] when W == 0) in its last; where several variants share a bubble they differ from each other in
both places too.  The graph, the coverages, the edit distances and the removals are written down here from the construction,
not computed; every edge comes with its reverse-complement twin, and the CPU test holds the edge lists to the oracle's
buildGraph of the same k-mer set.
"""
from oracle import pyref as R

import tips_cases as TC

K, J, G, C_G = TC.K, TC.J, TC.G, TC.C_G
edge, both, add_piece = TC.edge, TC.both, TC.add_piece

# G[29:37] = A | G T G A G A C: the variants below replace bases from G[J] = 'G' on


def strong_path(w):
    return G[J - K:J + w + K]


def variant_path(w, v):
    return G[J - K:J] + v + G[J + w:J + w + K]


def variant_piece(w, v):
    return G[J - K + 1:J] + v + G[J + w:J + w + K - 1]


def cov_strong(w):
    return (w + K + 1, C_G * (w + K + 1), C_G, C_G)


def cov_variant(v, c):
    return (len(v) + K + 1, 2 * C_G + (len(v) + K - 1) * c, min(c, C_G), max(c, C_G))


def bubble_case(name, w, variants, max_len, max_diff, removed, pairs, dist, pairs_at_0, extra=None):
    """variants: [(V, count)]; removed: the V's whose edges (and twins) go, "" = the genome's own branch; dist: {(V1, V2): the
    Levenshtein distance of the two edges, hand-counted}; pairs = pairs_compared at max_diff, pairs_at_0 at max_diff = 0"""
    counts = {}
    add_piece(counts, G, C_G)
    edges = both(G[:J]) + both(strong_path(w)) + both(G[J + w:])
    cov = {edge(strong_path(w)): cov_strong(w)}
    path_of = {"": strong_path(w)}
    for v, c in variants:
        add_piece(counts, variant_piece(w, v), c)
        edges += both(variant_path(w, v))
        cov[edge(variant_path(w, v))] = cov_variant(v, c)
        cov[edge(R.rev_comp(variant_path(w, v)))] = cov_variant(v, c)
        path_of[v] = variant_path(w, v)
    keep = []
    if extra:                                                # a tip at the same junction (tests/tips_cases.py: out_arm)
        piece, arm = extra
        add_piece(counts, piece, 2)
        edges += both(arm)
        keep = both(arm)
    rm = set()
    for v in removed:
        rm |= set(both(path_of[v]))
    d = {(edge(path_of[a]), edge(path_of[b])): n for (a, b), n in dist.items()}
    return dict(name=name, counts=counts, edges=edges, max_len=max_len, max_diff=max_diff, removed=rm, pairs=pairs, pairs_at_0=pairs_at_0,
                cov=cov, dist=d, keep=keep)


def cases():
    L1 = K + 1                                               # the length of both branches of a SNP bubble
    return [
        # G[J] = 'G' -> 'C': one substitution
        bubble_case("snp_weak_branch", 1, [("C", 2)], 2 * K, 3, ["C"], 2, {("", "C"): 1}, 2),
        bubble_case("snp_equal_coverage", 1, [("C", C_G)], 2 * K, 3, [], 2, {("", "C"): 1}, 2),          # a tie: both stay
        # W = 0: a 'C' inserted before G[J] (it differs from G[J] = 'G' and from G[J-1] = 'A'): K + 1 bases beside K
        bubble_case("insertion_in_weak_branch", 0, [("C", 3)], 2 * K, 3, ["C"], 2, {("", "C"): 1}, 0),
        # G[J:J+7] = GTGAGAC -> CTCATAG: four substitutions, a matching base between each two
        bubble_case("four_differences_at_3", 7, [("CTCATAG", 2)], 4 * K, 3, [], 2, {("", "CTCATAG"): 4}, 2),
        bubble_case("four_differences_at_4", 7, [("CTCATAG", 2)], 4 * K, 4, ["CTCATAG"], 2, {("", "CTCATAG"): 4}, 2),
        bubble_case("branch_at_max_len", 1, [("C", 2)], L1, 3, ["C"], 2, {("", "C"): 1}, 2),
        bubble_case("branch_over_max_len", 1, [("C", 2)], L1 - 1, 3, [], 0, {("", "C"): 1}, 0),
        # G[J:J+5] = GTGAG = g; f = CAGAT (3 from g: places 0, 1, 4); e = AACAC (3 from f: places 0, 2, 4; 4 from g: 0, 1, 2, 4).
        # e < f < g in coverage, d(e,f) <= 3, d(f,g) <= 3, d(e,g) > 3: e goes for f, f goes for g
        bubble_case("chain_of_three", 5, [("CAGAT", 4), ("AACAC", 2)], 2 * K, 3, ["CAGAT", "AACAC"], 6,
                    {("", "CAGAT"): 3, ("CAGAT", "AACAC"): 3, ("", "AACAC"): 4}, 6),
        # a SNP bubble and, at the same branch node, a dead-end arm of 4 bases (first base 'A'): pop leaves the tip alone
        bubble_case("bubble_next_to_a_tip", 1, [("C", 2)], 2 * K, 3, ["C"], 2, {("", "C"): 1}, 2, extra=TC.out_arm(4, 0)),
    ]
