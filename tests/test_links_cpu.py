"""The scaffold-link rules on the CPU: tests/links_ref.py (the restatement the GPU tests compare the device with) is held to
answers worked out by hand on a hand-written graph, one case per class and u counted on the genome's text; the twin identity is
checked by algebra on every pair of positions of that graph; gk_scaffold_chains (host code of the library, no GPU) is held to the
restatement's chains."""
import ctypes as C
import random

import numpy as np
import pytest

from genome_amd import _lib as L
from genome_amd import graph as G
from links_ref import CLASSES, JOIN_STATS, chains, classify, index_graph, joins, pair_links
from oracle import pyref as R

K = 4
# three edges, written out: path = start ++ sequence.  Edge 2 leaves edge 0's end node (GCCA).  No 4-mer occurs twice in them
# but that node's, none is another's reverse complement.
P0 = "CCTGAGTGCCTCCAGACGCAGCCA"          # edge 0: start CCTG, 20 bases, end GCCA
P1 = "CATAGCGGGACACGAT"                  # edge 1: start CATA, 12 bases, end CGAT
P2 = "GCCAATCTACGG"                      # edge 2: start GCCA (the end node of edge 0), 8 bases, end ACGG
PATHS = [P0, P1, P2]
EDGES = [(p[:K], p[K:]) for p in PATHS]
LENS = [20, 12, 8]
assert G.LINK_CLASSES == CLASSES and G.JOIN_STATS == JOIN_STATS


def pair(pa, a, pb, b):
    """a pair whose orientation 0 finds mate 1 at distance a of path pa and mate 2's reverse complement at distance b of pb"""
    return [pa[a:a + K], R.rev_comp(pb[b:b + K])]


def test_the_hand_graph_is_what_the_cases_assume():
    windows = [p[d:d + K] for p in PATHS for d in range(len(p) - K + 1)]
    assert len(windows) == 21 + 13 + 9 and len(set(windows)) == len(windows) - 1          # GCCA: the end of edge 0 and the start of edge 2
    assert not {R.rev_comp(w) for w in windows} & set(windows)
    index, lens = index_graph(K, EDGES)
    assert lens == LENS
    assert index["GCCA"] == [("N", sorted({"CCTG", "GCCA", "CATA", "CGAT", "ACGG"}).index("GCCA"))]
    assert index["TGAG"] == [("E", 0, 2)] and index["GGGA"] == [("E", 1, 6)] and index["ATCT"] == [("E", 2, 4)]


# min_len = 12 contig bases: k + len is 24, 16, 12 for the three edges.  max_span = 30.
HAND = [
    # the G = -k case: edge 2 leaves edge 0's end node.  u = (20 + 4 - 14) + (4 + 4) = 18
    (pair(P0, 14, P2, 4), 12, 30, "linked", (0, 2, 18)),
    (pair(P0, 2, P1, 5), 12, 30, "too_far", None),               # u = (20 + 4 - 2) + (5 + 4) = 31
    (pair(P0, 3, P1, 5), 12, 30, "linked", (0, 1, 30)),          # u = 21 + 9: the last one inside max_span
    (pair(P1, 11, P0, 1), 12, 30, "linked", (1, 0, 10)),         # the smallest u there is: the last edge position and the first
    (pair(P1, 11, P0, 1), 12, 9, "too_far", None),
    (pair(P0, 2, P0, 8), 12, 30, "same_edge", None),
    (pair(P0, 8, P0, 2), 0, 1 << 40, "same_edge", None),         # whatever the order on the edge
    (pair(P0, 0, P1, 5), 12, 30, "at_node", None),               # the start node's k-mer
    (pair(P1, 3, P0, 20), 12, 30, "at_node", None),              # the end node's, which is edge 2's start node too
    (pair(P0, 14, P2, 4), 13, 30, "short_edge", None),           # edge 2's contig has 12 bases
    (pair(P2, 4, P0, 14), 13, 100, "short_edge", None),          # either side
    (pair(P0, 14, P2, 4), 25, 30, "short_edge", None),           # edge 0's has 24
    (pair(P0, 2, P1, 5), 17, 30, "short_edge", None),            # short_edge is tested before too_far
    (["TTTT", R.rev_comp(P0[6:10])], 0, 30, "unplaced", None),
    ([P0[2:6], "AAAA"], 0, 30, "unplaced", None),
]


@pytest.mark.parametrize("case", range(len(HAND)))
def test_one_orientation_by_hand(case):
    (m1, m2), min_len, max_span, want, hit = HAND[case]
    index, lens = index_graph(K, EDGES)
    assert classify(index.get(m1, []), index.get(R.rev_comp(m2), []), K, lens, min_len, max_span) == (want, hit)


def test_u_is_the_fragment_less_the_gap():
    """Edges 0 and 2 share a node, so the genome reads P0 ++ P2[k:] and G = -k: a fragment from base da of P(0) to the end of the
    window at base db of P(2) has u - k bases, counted on the text."""
    genome = P0 + P2[K:]
    index, lens = index_graph(K, EDGES)
    for da in range(1, 20):
        for db in range(1, 8):
            m1, m2 = pair(P0, da, P2, db)
            cls, (e, f, u) = classify(index[m1], index[R.rev_comp(m2)], K, lens, 0, 1 << 20)
            assert (cls, e, f) == ("linked", 0, 2)
            frag = genome[da:da + u - K]
            assert frag[:K] == m1 and R.rev_comp(frag)[:K] == m2


def test_repetitive_by_hand():
    """two positions on either side are not looked at, whatever they are; unplaced is tested first"""
    idx, ln = index_graph(K, EDGES, nodes=["TTTT", "TTTT", "CCTG", "GCCA", "CATA", "CGAT", "ACGG"])
    assert len(idx["TTTT"]) == 2
    assert classify(idx["TTTT"], idx["TGAG"], K, ln, 0, 100) == ("repetitive", None)
    assert classify(idx["TGAG"], idx["TTTT"], K, ln, 0, 100) == ("repetitive", None)
    assert classify([("E", 0, 2), ("E", 1, 3)], [("E", 2, 4)], K, ln, 0, 100) == ("repetitive", None)
    assert classify([], idx["TTTT"], K, ln, 0, 100) == ("unplaced", None)


def twin_graph():
    """the three edges and their reverse complements: edge e + 3 is the twin of edge e"""
    paths = PATHS + [R.rev_comp(p) for p in PATHS]
    return paths, index_graph(K, [(p[:K], p[K:]) for p in paths])


def test_orientation_1_is_the_twin_link():
    """Every pair of edge positions on two different edges of the strand-closed hand graph: orientation 0 of the pair lands on
    (e, f), orientation 1 (the mates swapped) on (twin f, twin e), with the same u — and with the same class under any min_len and
    max_span."""
    paths, (index, lens) = twin_graph()
    twin = lambda e: (e + 3) % 6
    seen = 0
    for e in range(6):
        for f in range(6):
            if e == f:
                continue
            for da in range(1, lens[e]):
                for db in range(1, lens[f]):
                    m1, m2 = pair(paths[e], da, paths[f], db)
                    o0 = classify(index[m1], index[R.rev_comp(m2)], K, lens, 0, 1 << 20)
                    o1 = classify(index[m2], index[R.rev_comp(m1)], K, lens, 0, 1 << 20)
                    u = (lens[e] + K - da) + (db + K)
                    assert o0 == ("linked", (e, f, u)) and o1 == ("linked", (twin(f), twin(e), u))
                    for min_len, max_span in ((13, 1 << 20), (0, 25), (17, 20)):
                        assert classify(index[m1], index[R.rev_comp(m2)], K, lens, min_len, max_span)[0] == \
                               classify(index[m2], index[R.rev_comp(m1)], K, lens, min_len, max_span)[0]
                    seen += 1
    assert seen > 3000
    # a stream over it: the link table is strand-closed
    rnd = random.Random(7)
    reads = []
    for _ in range(200):
        e, f = rnd.sample(range(6), 2)
        reads += pair(paths[e], rnd.randrange(1, lens[e]), paths[f], rnd.randrange(1, lens[f]))
    links, cls = pair_links(K, index, lens, reads, 200, 13, 28)
    assert cls["linked"] > 20 and cls["too_far"] > 20 and cls["short_edge"] > 20 and cls["orientations"] == 400 == sum(cls[c] for c in CLASSES[1:])
    assert all(links[(twin(f), twin(e))] == v for (e, f), v in links.items())


def test_a_stream_of_the_hand_cases():
    """the cases that share min_len = 12 and max_span = 30 as one stream, with a short mate among them: orientation 1 of every pair
    looks up reverse complements, which the graph (one strand written out) does not hold: unplaced"""
    index, lens = index_graph(K, EDGES)
    cases = [h for h in HAND if h[1:3] == (12, 30)]
    reads = [m for h in cases for m in h[0]] + ["CCT", P0[8:12]] + pair(P0, 3, P1, 5)
    links, cls = pair_links(K, index, lens, reads, len(reads) // 2, 12, 30)
    assert links == {(0, 2): [1, 18], (0, 1): [2, 60], (1, 0): [1, 10]}
    assert cls == {"orientations": 16, "unplaced": 8, "repetitive": 0, "at_node": 2, "same_edge": 1, "short_edge": 0, "too_far": 1, "linked": 4}
    assert pair_links(K, index, lens, reads, 1, 12, 30)[1]["orientations"] == 2


# ---- joins and chains ---------------------------------------------------------------------------------------------------------------

def test_joins_with_a_fork_and_a_merge():
    links = {(1, 2): [5, 50], (2, 3): [3, 40],                 # a path 1 -> 2 -> 3
             (4, 5): [9, 90], (4, 6): [3, 30],                 # a fork at 4: neither is a join
             (7, 9): [4, 40], (8, 9): [4, 44],                 # a merge at 9: neither
             (10, 11): [2, 20],                                # below the support
             (12, 13): [3, 33], (12, 14): [2, 20],             # the second link out of 12 is not supported: (12, 13) is a join
             (6, 1): [7, 70]}                                  # into the path's head; 6 has another predecessor-less life as a fork target
    got, st = joins(links, 3)
    assert got == [(1, 2, 5, 50), (2, 3, 3, 40), (6, 1, 7, 70), (12, 13, 3, 33)]
    assert st == dict(links=10, supported=8, joins=4, forks=1, merges=1)
    assert joins(links, 10) == ([], dict(links=10, supported=0, joins=0, forks=0, merges=0))
    assert joins(links, 1)[1] == dict(links=10, supported=10, joins=4, forks=2, merges=1)
    assert chains([j[0] for j in got], [j[1] for j in got]) == ([[6, 1, 2, 3], [12, 13]], 0)


def test_chains_with_a_cycle_and_two_singletons_left_out():
    """ids 0..11; 5 and 8 are in no join and are not listed; 7 -> 3 -> 9 -> 7 is a cycle and starts at 3"""
    e1, e2 = [4, 7, 3, 9, 10, 2, 0], [2, 3, 9, 7, 11, 6, 1]
    got = chains(e1, e2)
    assert got == ([[0, 1], [3, 9, 7], [4, 2, 6], [10, 11]], 1)
    assert not {5, 8} & {m for c in got[0] for m in c}
    assert chains([5], [5]) == ([[5]], 1)                      # a link of an edge to itself is a cycle of one
    assert chains([], []) == ([], 0)
    assert chains([1, 1], [2, 3]) is None and chains([1, 2], [3, 3]) is None


def lib_chains(e1, e2, members_cap=None, chains_cap=None):
    n = len(e1)
    a, b = np.array(e1, np.uint32), np.array(e2, np.uint32)
    mcap, ccap = 2 * n if members_cap is None else members_cap, n if chains_cap is None else chains_cap
    members, off = np.full(mcap + 1, 0xdead, np.uint32), np.full(ccap + 2, 0xdead, np.uint64)
    nch, ncy = C.c_uint64(99), C.c_uint64(99)
    rc = L.lib().gk_scaffold_chains(L.ptr(a, C.c_uint32), L.ptr(b, C.c_uint32), n, L.ptr(members, C.c_uint32), mcap, L.ptr(off, C.c_uint64), ccap,
                                    C.byref(nch), C.byref(ncy))
    assert members[mcap] == 0xdead and off[ccap + 1] == 0xdead
    if rc != L.GK_OK:
        return rc, nch.value, ncy.value
    return [members[int(off[i]):int(off[i + 1])].tolist() for i in range(nch.value)], ncy.value


@pytest.mark.parametrize("seed", range(12))
def test_gk_scaffold_chains_against_the_restatement(seed):
    """random join lists over at most 200 ids: e1 and e2 are samples without repetition, so paths, cycles and self-joins all occur"""
    rnd = random.Random(seed)
    nid = rnd.choice([1, 2, 7, 50, 200])
    n = rnd.randint(0, nid)
    e1, e2 = rnd.sample(range(nid), n), rnd.sample(range(nid), n)
    if seed % 3 == 0 and n:                                    # some sparse 32-bit ids
        scale = (0xfffffffe // nid)
        e1, e2 = [x * scale for x in e1], [x * scale for x in e2]
    want = chains(e1, e2)
    assert lib_chains(e1, e2) == want
    assert G.scaffoldChains(e1, e2, with_cycles=True) == want and G.scaffoldChains(e1, e2) == want[0]
    total = sum(len(c) for c in want[0])
    assert total <= 2 * n and len(want[0]) <= n
    assert lib_chains(e1, e2, members_cap=total, chains_cap=len(want[0])) == want        # exactly enough room
    if want[0]:
        assert lib_chains(e1, e2, members_cap=total - 1) == (L.GK_E_CAPACITY, len(want[0]), want[1])
        assert lib_chains(e1, e2, chains_cap=len(want[0]) - 1) == (L.GK_E_CAPACITY, len(want[0]), want[1])


def test_some_seed_has_cycles_and_paths():
    kinds = set()
    for seed in range(12):
        rnd = random.Random(seed)
        nid = rnd.choice([1, 2, 7, 50, 200])
        n = rnd.randint(0, nid)
        got, ncy = chains(rnd.sample(range(nid), n), rnd.sample(range(nid), n))
        kinds |= {"cycle"} if ncy else set()
        kinds |= {"path"} if len(got) > ncy else set()
        kinds |= {"long"} if any(len(c) >= 4 for c in got) else set()
    assert kinds == {"cycle", "path", "long"}


def test_gk_scaffold_chains_refuses_what_is_no_join_list():
    assert lib_chains([1, 1], [2, 3])[0] == L.GK_E_INVALID
    assert lib_chains([1, 2], [3, 3])[0] == L.GK_E_INVALID
    assert lib_chains([1, 2, 1], [3, 4, 5])[:2] == (L.GK_E_INVALID, 0)
    with pytest.raises(L.GkError) as e:
        G.scaffoldChains([1, 1], [2, 3])
    assert e.value.code == L.GK_E_INVALID
    assert L.lib().gk_scaffold_chains(None, None, 3, None, 0, None, 0, None, None) == L.GK_E_INVALID
    assert lib_chains([], []) == ([], 0)
