"""Hand-written graphs for the weak-connection rule (tests/test_weak_cpu.py holds the restatement to them, tests/test_weak_gpu.py
the device).

Each case is built as tests/tips_cases.py builds its own: genomes at a high count plus a few short pieces at a low one, the way
a chimeric read, a dissimilar variant or a stray contig leaves its k-mers in the table; the graph, the coverage of the pieces
and the edges the rule removes are written down here from the construction, not computed.  An edge is the path it spells:
(path[:K], path[-K:], path[K:]); every edge comes with its reverse-complement twin.  K = tips_cases.K = 11.

A piece that joins base a - 1 of one sequence to base b of another has K - 1 windows of its own (each holds the joint); the edge
it makes runs from the node X[a-K:a] to the node Y[b:b+K], K bases long, and reads K + 1 windows: its two end nodes, at the
genomes' counts, and the K - 1 of the piece.  So with the genomes at C1 and C2 and the piece at c the edge has
sum = C1 + C2 + (K - 1) c over K + 1 = 12 windows, and "5 times the edge is below a genome edge of mean C" reads
5 (C1 + C2 + 10 c) < 12 C.
"""
from oracle import pyref as R

import tips_cases as TC

K = TC.K
G = TC.G                                                            # 56 bases
H = "CGTAAACAGAATTAGATAAGATAGAGCTGACGAGCAAAGTTCTTCCGGGACTCTCA"      # 56 bases; shares no 10-mer with G, TAIL or LONE on either strand
A = TC.J                  # the bridges leave G behind base A - 1: at the node G[A-K:A]
B = 20                    # ... and enter H at base B: at the node H[B:B+K]
B1, B2 = 12, 32           # two bridges from one junction
edge, both, add_piece = TC.edge, TC.both, TC.add_piece
STATS = ("candidates", "removed_ratio", "removed_floor_only", "removed")

assert len({G[A], H[B1], H[B2]}) == 3 and H[B] != G[A]              # the junction's ways out differ in their first base
assert G[A - 1] not in (H[B - 1], H[B1 - 1], H[B2 - 1])             # ... and the ways into H's nodes in their last


def bridge(b):
    """(the piece, the edge's path) of a read that follows G up to base A - 1 and goes on with H from base b"""
    return G[A - K + 1:A] + H[b:b + K - 1], G[A - K:A] + H[b:b + K]


def case(name, counts, edges, removed, stats, max_len=2 * K, ratio=5, floor=0, cov=None):
    return dict(name=name, counts=counts, edges=edges, removed=set(removed), stats=dict(zip(STATS, stats)), max_len=max_len, ratio=ratio,
                floor=floor, cov=cov or {})


def bridge_case(name, c1, c2, c, removed, stats, **kw):
    """G at c1 and H at c2, joined by one bridge at c: ten edges, of which only the bridge and its twin are connections by shape"""
    counts = {}
    add_piece(counts, G, c1)
    add_piece(counts, H, c2)
    piece, path = bridge(B)
    add_piece(counts, piece, c)
    edges = both(G[:A]) + both(G[A - K:]) + both(H[:B + K]) + both(H[B:]) + both(path)
    cov = {e: (K + 1, c1 + c2 + (K - 1) * c, c, max(c1, c2)) for e in both(path)}
    cov[edge(G[A - K:])] = (len(G) - A + 1, c1 * (len(G) - A + 1), c1, c1)
    cov[edge(H[:B + K])] = (B + 1, c2 * (B + 1), c2, c2)
    return case(name, counts, edges, both(path) if removed else [], stats, cov=cov, **kw)


def cases():
    out = [
        # 5 * (100 + 120 + 10) = 1150 < 12 * 100 = 1200 at G's end and < 1440 at H's: the bridge goes
        bridge_case("chimeric_bridge", 100, 120, 1, True, (2, 2, 0, 2)),
        # 5 * (100 + 120 + 20) = 1200 = 12 * 100: a tie with the weaker competitor, G's edge — kept (below H's edge or not)
        bridge_case("bridge_at_exactly_ratio", 100, 120, 2, False, (2, 0, 0, 0)),
        # ... which ratio 4 removes: 4 * 240 = 960 < 1200
        bridge_case("bridge_tie_under_ratio_4", 100, 120, 2, True, (2, 2, 0, 2), ratio=4),
        # 5 * (100 + 20 + 10) = 650 < 1200 at G's end, but not < 12 * 20 = 240 at H's: a strong competitor at one end only — kept
        bridge_case("bridge_strong_at_one_end", 100, 20, 1, False, (2, 0, 0, 0)),
        # the bridge is K = 11 bases long
        bridge_case("bridge_at_max_len", 100, 120, 1, True, (2, 2, 0, 2), max_len=K),
        bridge_case("bridge_over_max_len", 100, 120, 1, False, (0, 0, 0, 0), max_len=K - 1),
        # mean 230 / 12 < 20: (B) holds as well, and the edge counts under (A); the genomes' edges are far above the floor
        bridge_case("bridge_under_both_rules", 100, 120, 1, True, (2, 2, 0, 2), floor=20),
        bridge_case("ratio_off_floor_on", 100, 120, 1, True, (2, 0, 2, 2), ratio=0, floor=20),
        bridge_case("both_rules_off", 100, 120, 1, False, (2, 0, 0, 0), ratio=0, floor=0),
    ]
    # an out-tip of low coverage (tips_cases' y_weak_arm): its end has in-degree 1 — no connection, (A) leaves it to the tip rule
    y = TC.cases()[0]
    assert y["name"] == "y_weak_arm"
    out.append(case("low_coverage_out_tip", y["counts"], y["edges"], [], (0, 0, 0, 0)))
    # a bubble whose weak arm replaces 6 bases of G by 6 others (edit distance 5 > max_diff 2: popBubbles keeps it).  Both arms run from
    # G[P-K:P] to G[P+M:P+M+K], M + K = 17 bases, 18 windows; the weak arm's K - 1 + M = 16 own windows are at 1:
    # 5 * (100 + 100 + 16) * 18 = 19440 < 100 * 18 * 18 = 32400
    P, M, c1 = 20, 6, 100
    alt = "".join(TC._other(b, i % 3) for i, b in enumerate(G[P:P + M]))
    weak_arm = G[P - K:P] + alt + G[P + M:P + M + K]
    counts = {}
    add_piece(counts, G, c1)
    add_piece(counts, weak_arm[1:-1], 1)
    out.append(case("dissimilar_bubble_arm", counts, both(G[:P]) + both(G[P - K:P + M + K]) + both(weak_arm) + both(G[P + M:]), both(weak_arm), (4, 2, 0, 2),
                    cov={edge(weak_arm): (M + K + 1, 2 * c1 + (K - 1 + M), 1, c1), edge(G[P - K:P + M + K]): (M + K + 1, c1 * (M + K + 1), c1, c1)}))
    # a weak self-loop at the through-node X = G[S:S+K]: X, three bases, X again.  14 bases, 15 windows, 13 of its own at 1:
    # 5 * (200 + 13) = 1065 < 100 * 15 = 1500 against G's way out of X and against G's way into X
    S = 22
    X = G[S:S + K]
    inner = TC._other(G[S + K]) + "C" + TC._other(G[S - 1])
    loop = X + inner + X
    counts = {}
    add_piece(counts, G, c1)
    add_piece(counts, loop[1:-1], 1)
    out.append(case("weak_self_loop", counts, both(G[:S + K]) + both(G[S:]) + both(loop), both(loop), (2, 2, 0, 2),
                    cov={edge(loop): (len(inner) + K + 1, 2 * c1 + len(inner) + K - 1, 1, c1)}))
    # two weak bridges leave G at one junction (three ways out) for two places of H: both go.  5 * 230 < 1200 for each
    counts = {}
    add_piece(counts, G, 100)
    add_piece(counts, H, 120)
    (p1, path1), (p2, path2) = bridge(B1), bridge(B2)
    add_piece(counts, p1, 1)
    add_piece(counts, p2, 1)
    out.append(case("two_bridges_at_one_junction", counts,
                    both(G[:A]) + both(G[A - K:]) + both(H[:B1 + K]) + both(H[B1:B2 + K]) + both(H[B2:]) + both(path1) + both(path2),
                    both(path1) + both(path2), (4, 4, 0, 4), cov={edge(path1): (K + 1, 230, 1, 120), edge(path2): (K + 1, 230, 1, 120)}))
    # an isolated contig at 1 beside G at 10: no connection, (A) keeps it; its mean, 1, is below a floor of 2
    counts = {}
    add_piece(counts, G, TC.C_G)
    add_piece(counts, TC.LONE, 1)
    lone = both(G) + both(TC.LONE)
    out.append(case("lone_contig_ratio_only", counts, lone, [], (0, 0, 0, 0), cov={edge(TC.LONE): (4, 4, 1, 1)}))
    out.append(case("lone_contig_under_floor", counts, lone, both(TC.LONE), (0, 0, 2, 2), floor=2))
    out.append(case("lone_contig_at_the_floor", counts, lone, [], (0, 0, 0, 0), floor=1))            # 4 < 1 * 4 does not hold
    return out
