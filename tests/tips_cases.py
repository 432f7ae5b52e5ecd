"""Hand-written graphs for the tip rule (tests/test_tips_cpu.py holds the restatement to them, tests/test_tips_gpu.py the device).

Each case is a genome G (count 10) plus a few short pieces that leave or enter it the way a sequencing error near a read end
does; the graph, the coverage of the arms and the edges the rule removes are written down here from the construction, not
computed.  An edge is the path it spells: (path[:k], path[-k:], path[k:]); every edge comes with its reverse-complement twin.
k = 11 is odd (no k-mer is its own reverse complement) and the sequences below share no 10-mer by accident: the CPU test holds
the edge lists to the oracle's buildGraph of the same k-mer set.
"""
from oracle import pyref as R

K = 11
J = 30          # the position of G whose base the pieces replace
G = "GATTGCACCGTATCAGGCTTACGAACTCCAGTGAGACGTTTGCGCATAAGTCGGAT"
TAIL = "CCTAGTCGAAGCTAGGATCCTAGCA"       # what follows an error base in an arm (or precedes it in an in-tip)
LONE = "TTGACCTGGAGCAA"                  # an isolated contig of k + 3 bases
C_G = 10


def _other(base, i=0):
    return [b for b in "AGCT" if b != base][i]


def edge(path):
    return (path[:K], path[-K:], path[K:])


def both(path):
    return [edge(path), edge(R.rev_comp(path))]


def add_piece(counts, seq, c):
    for i in range(len(seq) - K + 1):
        key = R.canon(seq[i:i + K])
        counts[key] = counts.get(key, 0) + c


def out_arm(t, which=0):
    """the piece of a read that ends t bases after an error at G[J]: its t windows all hold the error base; the arm's path starts
    one base earlier, at the junction G[J-K:J]"""
    tail = TAIL if which == 0 else TAIL[::-1]
    piece = G[J - K + 1:J] + _other(G[J], which) + tail[:t - 1]
    return piece, G[J - K] + piece


def y_case(name, t, c_arm, max_len, removed):
    """G, and one arm of t bases leaving it at G[J-K:J]"""
    counts = {}
    add_piece(counts, G, C_G)
    piece, arm = out_arm(t)
    add_piece(counts, piece, c_arm)
    edges = both(G[:J]) + both(G[J - K:]) + both(arm)
    cov = {edge(arm): (t + 1, C_G + t * c_arm, min(C_G, c_arm), max(C_G, c_arm)),
           edge(R.rev_comp(arm)): (t + 1, C_G + t * c_arm, min(C_G, c_arm), max(C_G, c_arm)),
           edge(G[:J]): (J - K + 1, C_G * (J - K + 1), C_G, C_G)}
    rm = set(both(arm)) if removed else set()
    return dict(name=name, counts=counts, edges=edges, max_len=max_len, removed=rm, cov=cov)


def cases():
    out = [
        y_case("y_weak_arm", 4, 2, 2 * K, True),
        y_case("y_equal_coverage", 4, C_G, 2 * K, False),            # a tie removes nothing
        y_case("arm_at_max_len", 6, 2, 6, True),
        y_case("arm_over_max_len", 6, 2, 5, False),
        y_case("arm_of_one_base", 1, 3, 2 * K, True),
    ]
    # an in-tip: a read that STARTS t bases before an error at G[J]; it enters G at G[J+1:J+K+1]
    t = 5
    piece = TAIL[:t - 1] + _other(G[J]) + G[J + 1:J + K]
    arm = piece + G[J + K]
    counts = {}
    add_piece(counts, G, C_G)
    add_piece(counts, piece, 3)
    out.append(dict(name="in_tip", counts=counts, edges=both(G[:J + K + 1]) + both(G[J + 1:]) + both(arm), max_len=2 * K,
                    removed=set(both(arm)), cov={edge(arm): (t + 1, C_G + 3 * t, 3, C_G)}))
    # two tips at one junction beside the strong edge: both go; an isolated short contig stays
    counts = {}
    add_piece(counts, G, C_G)
    p1, a1 = out_arm(4, 0)
    p2, a2 = out_arm(3, 1)
    add_piece(counts, p1, 2)
    add_piece(counts, p2, 3)
    add_piece(counts, LONE, 1)
    out.append(dict(name="two_tips_and_a_lone_contig", counts=counts,
                    edges=both(G[:J]) + both(G[J - K:]) + both(a1) + both(a2) + both(LONE), max_len=2 * K,
                    removed=set(both(a1) + both(a2)),
                    cov={edge(a1): (5, C_G + 8, 2, C_G), edge(a2): (4, C_G + 9, 3, C_G), edge(LONE): (4, 4, 1, 1)}))
    return out
