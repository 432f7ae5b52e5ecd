"""Hand-computed cases that hold tests/thread_ref.py, the restatement of gk_graph_thread_reads' rule (include/genome_amd.h), at
k = 5.  The graphs are one strand only unless a case says otherwise, so the reverse-complement strand of every read is
off_graph throughout (each case's numbers say so) and the forward strand can be followed by hand.  No device, no library."""
from collections import Counter

from oracle import pyref as R
from thread_ref import STATS, thread_reads, twin_edges

K = 5


def stats(**kw):
    st = dict.fromkeys(STATS, 0)
    st.update(kw)
    assert st["inner_windows"] == sum(st[c] for c in STATS[2:])
    return st


# a 2-in / 2-out node X = CTGAC: e0 = AACCA -> X, e1 = GTGGA -> X, e2 = X -> AGGTT, e3 = X -> TCCAA
X_NODES = ["AACCA", "GTGGA", "CTGAC", "AGGTT", "TCCAA"]
X_EDGES = [(0, 2, "TCTGAC"), (1, 2, "ACTGAC"), (2, 3, "AGGTT"), (2, 4, "TCCAA")]
# AACCA TCTGAC AGGTT without its first and last base: windows 0..4 on e0 (distances 1..5), window 5 = X, windows 6..9 on e2
READ_02 = "ACCATCTGACAGGT"
READ_13 = "TGGAACTGACTCCA"


def test_straight_path_is_all_on_edge():
    nodes, edges = ["ACGTA", "CAGAT"], [(0, 1, "GGCTTCAGAT")]
    sup, st = thread_reads(K, nodes, edges, ["CGTAGGCTTCAGA"])          # distances 1..9 of the one edge: 9 windows, 7 inner
    assert not sup
    assert st == stats(records=1, inner_windows=14, off_graph=7, on_edge=7)


def test_two_reads_on_different_branches():
    sup, st = thread_reads(K, X_NODES, X_EDGES, [READ_02, READ_13])
    assert sup == Counter({(0, 2): 1, (1, 3): 1})
    assert st == stats(records=2, inner_windows=32, off_graph=16, on_edge=14, crossings=2)


def test_length_one_edge_on_entry_and_on_exit_side():
    # TTACC -ACGGT-> u = ACGGT -A-> v = CGGTA -GCAAT-> GCAAT: at u the exit edge has length 1, at v the entry edge has
    nodes = ["TTACC", "ACGGT", "CGGTA", "GCAAT"]
    edges = [(0, 1, "ACGGT"), (1, 2, "A"), (2, 3, "GCAAT")]
    sup, st = thread_reads(K, nodes, edges, ["TACCACGGTAGCAA"])         # windows 4 and 5 are u and v
    assert sup == Counter({(0, 1): 1, (1, 2): 1})
    assert st == stats(records=1, inner_windows=16, off_graph=8, on_edge=6, crossings=2)
    # each side on its own: a read that ends on v (its last window) crosses u only, one that starts on u crosses v only
    assert thread_reads(K, nodes, edges, ["TACCACGGTA"])[0] == Counter({(0, 1): 1})
    assert thread_reads(K, nodes, edges, ["ACGGTAGCAA"])[0] == Counter({(1, 2): 1})


def test_three_node_windows_in_a_row():
    nodes = ["TTACC", "ACGGT", "CGGTA", "GGTAG", "CAATC"]
    edges = [(0, 1, "ACGGT"), (1, 2, "A"), (2, 3, "G"), (3, 4, "CAATC")]
    sup, st = thread_reads(K, nodes, edges, ["TACCACGGTAGCAAT"])        # windows 4, 5, 6 are nodes
    assert sup == Counter({(0, 1): 1, (1, 2): 1, (2, 3): 1})
    assert st == stats(records=1, inner_windows=18, off_graph=9, on_edge=6, crossings=3)


def test_self_loop_crossed_twice_counts_two():
    # TTTCA -TACCTC-> X = ACCTC, the loop X -GGACCTC-> X, X -AATGG-> AATGG; three times round the loop: X is crossed four times
    nodes = ["TTTCA", "ACCTC", "AATGG"]
    edges = [(0, 1, "TACCTC"), (1, 1, "GGACCTC"), (1, 2, "AATGG")]
    full = "TTTCA" + "TACCTC" + "GGACCTC" * 3 + "AATGG"
    sup, st = thread_reads(K, nodes, edges, [full[1:-1]])
    assert sup == Counter({(0, 1): 1, (1, 1): 2, (1, 2): 1})
    assert st == stats(records=1, inner_windows=58, off_graph=29, on_edge=25, crossings=4)


def test_wrong_base_before_at_and_after_the_node():
    def run(pos, base):
        assert READ_02[pos] != base
        return thread_reads(K, X_NODES, X_EDGES, [READ_02[:pos] + base + READ_02[pos + 1:]])
    # before (base 4, the last of the entry window): windows 0..4 are off the graph, X has no entry
    sup, st = run(4, "G")
    assert not sup and st == stats(records=1, inner_windows=16, off_graph=8 + 4, on_edge=3, broken=1)
    # at the node (base 7): windows 3..7 are off the graph, no window is a node
    sup, st = run(7, "A")
    assert not sup and st == stats(records=1, inner_windows=16, off_graph=8 + 5, on_edge=3)
    # after (base 10, the exit base): X has no out-edge by C, windows 6..9 are off the graph
    sup, st = run(10, "C")
    assert not sup and st == stats(records=1, inner_windows=16, off_graph=8 + 3, on_edge=4, broken=1)
    # the exit base changed into the OTHER branch's: the read does leave by e3 for one window, and that is what is counted
    sup, st = run(10, "T")
    assert sup == Counter({(0, 3): 1}) and st == stats(records=1, inner_windows=16, off_graph=8 + 2, on_edge=5, crossings=1)


def test_shortest_reads():
    assert thread_reads(K, X_NODES, X_EDGES, ["CTGACA", "TCTGAC", "CTGAC", "", "A"]) == (Counter(), stats())      # k + 1 and below: skipped
    sup, st = thread_reads(K, X_NODES, X_EDGES, ["TCTGACA"])             # k + 2: X is the one inner window
    assert sup == Counter({(0, 2): 1})
    assert st == stats(records=1, inner_windows=2, off_graph=1, crossings=1)


def test_a_node_with_a_copy_is_repeated():
    # after a split: X keeps e0 and e2, its copy (node 5) gets e1 and e3; the k-mer CTGAC now has two positions
    nodes = X_NODES + ["CTGAC"]
    edges = [(0, 2, "TCTGAC"), (1, 5, "ACTGAC"), (2, 3, "AGGTT"), (5, 4, "TCCAA")]
    sup, st = thread_reads(K, nodes, edges, [READ_02, READ_13])
    assert not sup
    assert st == stats(records=2, inner_windows=32, off_graph=16, repeated=2, on_edge=14)


def strand_closed(nodes, edges):
    """the graph plus its reverse complement"""
    nodes2 = nodes + [R.rev_comp(s) for s in nodes]
    n = len(nodes)
    edges2 = list(edges)
    for s, t, q in edges:
        path = R.rev_comp(nodes[s] + q)
        edges2.append((n + t, n + s, path[K:]))
    return nodes2, edges2


def test_twin_symmetry():
    nodes, edges = strand_closed(X_NODES, X_EDGES)
    assert len(set(nodes)) == len(nodes)
    twin = twin_edges(K, nodes, edges)
    reads = [READ_02, READ_02, READ_13]
    sup, st = thread_reads(K, nodes, edges, reads)
    assert sup == Counter({(0, 2): 2, (twin[2], twin[0]): 2, (1, 3): 1, (twin[3], twin[1]): 1})
    assert all(sup[(twin[f], twin[e])] == c for (e, f), c in sup.items())
    assert st == stats(records=3, inner_windows=48, on_edge=42, crossings=6)
    # a read and its reverse complement are the same evidence
    assert thread_reads(K, nodes, edges, [R.rev_comp(r) for r in reads]) == (sup, st)
