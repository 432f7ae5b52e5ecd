"""The insert-range rules on the CPU: tests/insert_ref.py (the restatement the GPU tests compare the device with) is held to
answers worked out by hand on hand-written graphs, one case per class and both sides of the near_end boundary; gk_insert_range
(host code of the library, no GPU) is held to the restatement's integers."""
import ctypes as C
import random

import numpy as np
import pytest

from genome_amd import _lib as L
from genome_amd import graph as G
from insert_ref import CLASSES, classify, index_graph, insert_range, pair_distances
from oracle import pyref as R

K = 4
# two edges, written out: path = start ++ sequence.  No 4-mer occurs twice in them, none is another's reverse complement.
P0 = "CCTGAGTGCCTCCAGACGCAGCCA"          # edge 0: start CCTG, 20 bases, end GCCA
P1 = "CATAGCGGGACACGAT"                  # edge 1: start CATA, 12 bases, end CGAT
EDGES = [(P0[:K], P0[K:]), (P1[:K], P1[K:])]


def pair(pa, a, pb, b):
    """a pair whose orientation 0 finds mate 1 at distance a of path pa and mate 2's reverse complement at distance b of pb"""
    return [pa[a:a + K], R.rev_comp(pb[b:b + K])]


def test_the_hand_graph_is_what_the_cases_assume():
    windows = [p[d:d + K] for p in (P0, P1) for d in range(len(p) - K + 1)]
    assert len(windows) == len(set(windows)) == 21 + 13
    assert not {R.rev_comp(w) for w in windows} & set(windows)
    index, lens = index_graph(K, EDGES)
    assert lens == [20, 12]
    assert index["TGAG"] == [("E", 0, 2)] and index["CCTC"] == [("E", 0, 8)] and index["GGGA"] == [("E", 1, 6)]
    assert index["CCTG"][0][0] == "N" and index["GCCA"][0][0] == "N" and len(index["GCCA"]) == 1      # distance 0 and distance len: nodes
    assert sum(len(v) for v in index.values()) == 4 + 19 + 11


# bins = 13: max_dist = 12.  near_end on edge 0 (20 bases): dist(a) + 12 - 4 >= 20, i.e. dist(a) >= 12; on edge 1 (12 bases): dist(a) >= 4.
HAND = [
    (pair(P0, 2, P0, 8), "counted", 10),         # D = 8 - 2 + 4
    (pair(P0, 11, P0, 13), "counted", 6),        # the last accepted dist(a) on edge 0: 11 + 8 = 19 < 20
    (pair(P0, 12, P0, 14), "near_end", 6),       # the first rejected one: 12 + 8 = 20
    (pair(P1, 3, P1, 5), "counted", 6),          # edge 1: 3 + 8 = 11 < 12
    (pair(P1, 4, P1, 6), "near_end", 6),         # 4 + 8 = 12
    (pair(P0, 3, P0, 3), "counted", 4),          # both mates' k-mers the same window: D = k, the shortest fragment
    (pair(P0, 1, P0, 10), "beyond", 13),         # D = 13 > 12
    (pair(P0, 8, P0, 2), "reversed", -2),
    (pair(P0, 5, P0, 4), "reversed", 3),         # D = k - 1
    (pair(P0, 2, P1, 5), "apart", None),         # two edges
    (pair(P0, 0, P0, 6), "apart", None),         # the start node's k-mer is a node position: no edge combination
    (pair(P0, 20, P0, 6), "apart", None),        # so is the end node's
    (["TTTT", R.rev_comp(P0[6:10])], "unplaced", None),
    ([P0[2:6], "AAAA"], "unplaced", None),
]


@pytest.mark.parametrize("case", range(len(HAND)))
def test_one_orientation_by_hand(case):
    (m1, m2), want, D = HAND[case]
    index, lens = index_graph(K, EDGES)
    got = classify(index.get(m1, []), index.get(R.rev_comp(m2), []), K, lens, 12)
    assert got == (want, D)


def test_a_stream_of_the_hand_cases():
    """All of them as one stream, with a short mate among them: orientation 1 of every pair looks up reverse complements, which
    the graph (one strand written out) does not hold: unplaced."""
    index, lens = index_graph(K, EDGES)
    reads = [m for (p, _, _) in HAND for m in p] + ["CCT", P0[8:12]] + pair(P0, 2, P0, 8)
    hist, cls = pair_distances(K, index, lens, reads, len(reads) // 2, 13)
    want_hist = [0] * 13
    want_hist[10], want_hist[6], want_hist[4] = 2, 2, 1
    assert hist == want_hist
    assert cls == {"orientations": 30, "unplaced": 15 + 2, "repetitive": 0, "apart": 3, "ambiguous": 0, "reversed": 2, "beyond": 1, "near_end": 2,
                   "counted": 5}
    assert cls["orientations"] == sum(cls[c] for c in CLASSES[1:])
    # npairs below the stream: the first pair only
    assert pair_distances(K, index, lens, reads, 1, 13)[1]["orientations"] == 2
    # bins is part of the rule.  max_dist = 9: the two D = 10 pairs join the D = 13 one in beyond; near the end is dist(a) >= 15 on
    # edge 0 and dist(a) >= 7 on edge 1, so all four D = 6 pairs are counted
    hist9, cls9 = pair_distances(K, index, lens, reads, len(reads) // 2, 10)
    assert cls9["beyond"] == 3 and cls9["near_end"] == 0 and cls9["counted"] == 5
    assert hist9 == [0, 0, 0, 0, 1, 0, 4, 0, 0, 0]


def test_ambiguous_and_repetitive_by_hand():
    """One edge in which CTGA occurs at distances 1 and 9, and CCTG as the start node and at distance 8."""
    path = "CCTGAGTGCCTGAGACG"                   # start CCTG, 13 bases
    edges = [(path[:K], path[K:])]
    index, lens = index_graph(K, edges)
    assert index["CTGA"] == [("E", 0, 1), ("E", 0, 9)] and index["GACG"] == [("N", 1)] and index["AGAC"] == [("E", 0, 12)]
    assert classify(index["CTGA"], index["AGAC"], K, lens, 64) == ("ambiguous", None)           # two combinations on the one edge
    assert index["CCTG"] == [("N", 0), ("E", 0, 8)]
    assert classify(index["CCTG"], index["AGAC"], K, lens, 7) == ("beyond", 8)                  # one combination (the node entry pairs with nothing): D = 12 - 8 + 4
    assert classify(index["CCTG"], index["AGAC"], K, lens, 8) == ("counted", 8)                 # 8 + 8 - 4 = 12 < 13
    assert classify(index["CCTG"], index["AGAC"], K, lens, 9) == ("near_end", 8)                # 8 + 9 - 4 = 13 >= 13
    # 16 entries are looked at, 17 are not
    for copies, want in ((16, "apart"), (17, "repetitive")):
        idx, ln = index_graph(K, edges, nodes=["TTTT"] * copies + ["CCTG", "GACG"])
        assert len(idx["TTTT"]) == copies
        assert classify(idx["TTTT"], idx["AGAC"], K, ln, 64)[0] == want
        assert classify(idx["AGAC"], idx["TTTT"], K, ln, 64)[0] == want
    assert classify([], [("N", 0)] * 17, K, lens, 64)[0] == "unplaced"                           # unplaced is tested first


# ---- gk_insert_range against the restatement ------------------------------------------------------------------------------------

def lib_range(hist, trim, min_obs):
    h = np.ascontiguousarray(hist, np.uint64)
    lo, hi, med = C.c_uint32(7), C.c_uint32(7), C.c_uint32(7)
    rc = L.lib().gk_insert_range(L.ptr(h, C.c_uint64), len(h), trim, min_obs, C.byref(lo), C.byref(hi), C.byref(med))
    return rc, (lo.value, hi.value, med.value)


def test_insert_range_by_hand():
    h = [0, 0, 0, 10, 20, 40, 20, 10, 0, 0]                  # n = 100
    assert insert_range(h, 0, 1) == (3, 7, 5)
    assert insert_range(h, 100, 1) == (4, 6, 5)              # ties at a bin edge: 1000 * 10 > 100 * 100 is false at D = 3, lo moves on;
                                                             # 1000 * 90 >= 900 * 100 holds at D = 6, hi stays
    assert insert_range(h, 99, 1) == (3, 7, 5)               # one thousandth less: 10000 > 9900 at D = 3; 90000 >= 90100 fails at D = 6
    assert insert_range(h, 300, 1) == (5, 5, 5)              # cum(4) = 30: 30000 > 30000 is false; cum(5) = 70: 70000 >= 70000 holds
    assert insert_range(h, 499, 1) == (5, 5, 5)
    assert insert_range(h, 25, 101) == (0, 0, 0)
    assert insert_range([0, 0, 5, 0], 25, 1) == (2, 2, 2)    # a single occupied bin


@pytest.mark.parametrize("trim", [0, 25, 100, 499])
def test_insert_range_matches_the_restatement(trim):
    rnd = random.Random(trim)
    for case in range(60):
        bins = rnd.choice([2, 3, 17, 512, 4096])
        hist = [0] * bins
        for _ in range(rnd.choice([1, 3, 40, 1000])):
            hist[min(bins - 1, max(0, int(rnd.gauss(bins / 2, bins / 10))))] += rnd.choice([1, 1, 2, 1000, 2 ** 40])
        for min_obs in (0, 1, 1000, sum(hist), sum(hist) + 1):
            rc, got = lib_range(hist, trim, min_obs)
            assert rc == L.GK_OK and got == insert_range(hist, trim, min_obs), (hist, trim, min_obs)
    # ties at a bin edge: n = 1000, so trim thousandths are whole observations
    hist = [0, 25, 950, 25, 0]
    assert lib_range(hist, 25, 1)[1] == insert_range(hist, 25, 1) == (2, 2, 2)
    assert lib_range(hist, 24, 1)[1] == insert_range(hist, 24, 1) == (1, 3, 2)
    assert lib_range(hist, 0, 1)[1] == (1, 3, 2)
    assert lib_range([0, 1, 1, 0], 0, 1)[1] == (1, 2, 1)     # 2 * cum >= n at the lower of two middle bins
    # counts whose sum passes 2^64 are compared exactly
    big = [2 ** 63, 2 ** 63, 2 ** 63, 1]
    assert lib_range(big, 0, 1)[1] == insert_range(big, 0, 1) == (0, 3, 1)


def test_insert_range_no_estimate_and_invalid_arguments():
    assert lib_range([0] * 8, 25, 0) == (L.GK_OK, (0, 0, 0))             # n = 0 is below max(0, 1)
    assert lib_range([0, 0, 999, 0], 25, 1000) == (L.GK_OK, (0, 0, 0))
    assert lib_range([0, 0, 1000, 0], 25, 1000) == (L.GK_OK, (2, 2, 2))
    lib = L.lib()
    h = np.ones(8, np.uint64)
    out = C.c_uint32()
    assert lib.gk_insert_range(L.ptr(h, C.c_uint64), 8, 500, 1, C.byref(out), None, None) == L.GK_E_INVALID
    assert lib.gk_insert_range(None, 8, 25, 1, C.byref(out), None, None) == L.GK_E_INVALID
    assert lib.gk_insert_range(L.ptr(h, C.c_uint64), 1, 25, 1, C.byref(out), None, None) == L.GK_E_INVALID
    big = np.ones(65537, np.uint64)
    assert lib.gk_insert_range(L.ptr(big, C.c_uint64), 65537, 25, 1, C.byref(out), None, None) == L.GK_E_INVALID
    assert lib.gk_insert_range(L.ptr(big, C.c_uint64), 65536, 25, 1, None, None, None) == L.GK_OK      # any output may be NULL
    # the Python wrapper: None for "no estimate", a triple otherwise
    assert G.insertRange([0, 0, 999, 0]) is None
    assert G.insertRange([0, 0, 1000, 0]) == (2, 2, 2)
    assert G.insertRange([0, 3, 0, 4], trim=0, min_observations=1) == (1, 3, 3)
    with pytest.raises(L.GkError):
        G.insertRange([1, 2, 3], trim=500)
