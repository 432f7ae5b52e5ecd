"""The restatement of the gap-filling rule (tests/fillgaps_ref.py) held to hand-computed cases, and its strand symmetry on the
oracle's graph of insert_cases.small_pairs.  No GPU.  Graphs are {edge id: (start node, end node, len)}; k = 5 throughout the
hand cases, so a filler of S bases has gap length L = S - 5."""
import random

import pytest

import fillgaps_cases as FC
import fillgaps_ref as FR
import scaffolds_cases as SC
from insert_cases import small_pairs

K = 5
# contig 0 into node 1, contig 2 out of node 2 (3 likewise, for a second junction between the same nodes)
BASE = {0: (0, 1, 50), 2: (2, 3, 50)}


def run(edges, chains, gaps, tol=0, **kw):
    c, g, rep = FR.fill(edges, K, chains, gaps, tol, **kw)
    assert rep["junctions"] == sum(rep[n] for n in FR.STATS[1:7]) == sum(len(x) - 1 for x in chains)
    assert [len(x) - 1 for x in c] == [len(x) for x in g] and sum(len(x) for x in c) == sum(len(x) for x in chains) + rep["filler_edges"]
    return c, g, rep


def one(edges, G, tol=0, **kw):
    """the class of the junction 0 -> 2, and the filled chain"""
    c, g, rep = run(edges, [[0, 2]], [[G]], tol, **kw)
    return rep["classes"][0][0], c[0], g[0], rep


def test_one_filler():
    edges = {**BASE, **{1: (1, 2, 7)}}
    cls, chain, gaps, rep = one(edges, 2)
    assert (cls, chain, gaps) == ("filled", [0, 1, 2], [-K, -K])
    assert rep["lengths"] == [[2]] and (rep["filled"], rep["filler_edges"], rep["filler_bases"], rep["searched_backward"]) == (1, 1, 7, 0)
    # adjacent: nothing is searched, the gap is not looked at
    c, g, rep = run(edges, [[0, 1, 2]], [[99, -99]])
    assert (c, g, rep["classes"], rep["adjacent"]) == ([[0, 1, 2]], [[99, -99]], [["adjacent", "adjacent"]], 2)
    # a chain of one member has no junction
    assert run(edges, [[1]], [[]])[2]["junctions"] == 0


def test_max_edges():
    edges = {**BASE, **{10: (1, 11, 4), 11: (11, 12, 4), 12: (12, 2, 4)}}
    assert one(edges, 7, max_edges=3)[:3] == ("filled", [0, 10, 11, 12, 2], [-K] * 4)
    assert one(edges, 7, max_edges=2)[0] == "none"
    longer = {**BASE, **{10: (1, 11, 4), 11: (11, 12, 4), 12: (12, 13, 4), 13: (13, 2, 4)}}
    assert one(longer, 11, max_edges=3)[0] == "none" and one(longer, 11, max_edges=4)[0] == "filled"


def test_the_window_is_closed_at_both_ends():
    edges = {**BASE, **{1: (1, 2, 15)}}                    # L = 10
    assert [one(edges, G, tol=2)[0] for G in (7, 8, 10, 12, 13)] == ["none", "filled", "filled", "filled", "none"]
    assert one(edges, 8, tol=2)[3]["lengths"] == [[10]]


def test_a_negative_gap_length_and_an_empty_bound():
    edges = {**BASE, **{1: (1, 2, 2)}}                     # S = 2 < k: L = -3, the contigs overlap by three bases
    cls, chain, gaps, rep = one(edges, -3)
    assert (cls, chain, gaps, rep["lengths"]) == ("filled", [0, 1, 2], [-K, -K], [[-3]])
    assert one(edges, -4)[0] == "none" and one(edges, -4, tol=1)[0] == "filled"
    assert one(edges, -10)[0] == "none"                      # B = -5
    assert one(edges, -5)[0] == "none" and one(edges, -5, tol=1)[0] == "none"      # B = 0 and B = 1: nothing of S = 2 fits


def test_a_bubble_is_ambiguous():
    edges = {**BASE, **{1: (1, 2, 7), 4: (1, 2, 7)}}
    cls, chain, gaps, rep = one(edges, 2)
    assert (cls, chain, gaps, rep["lengths"], rep["ambiguous"]) == ("ambiguous", [0, 2], [2], [[0]], 1)
    edges[4] = (1, 2, 8)                                     # two lengths: one hit at tol 0, two at tol 1
    assert one(edges, 2)[0] == "filled" and one(edges, 3)[1] == [0, 4, 2] and one(edges, 2, tol=1)[0] == "ambiguous"


def test_an_edge_twice_on_the_path_is_shared():
    edges = {**BASE, **{5: (1, 1, 3), 6: (1, 2, 4)}}       # a loop at node 1: the paths 6, 5 6, 5 5 6 of L = -1, 2, 5
    assert one(edges, -1)[:2] == ("filled", [0, 6, 2]) and one(edges, 2)[:2] == ("filled", [0, 5, 6, 2])
    cls, chain, gaps, rep = one(edges, 5)
    assert (cls, chain, gaps, rep["lengths"], rep["shared"], rep["filler_edges"]) == ("shared", [0, 2], [5], [[5]], 1, 0)


def test_contested_edges_lose_on_every_side():
    edges = {**BASE, **{1: (1, 2, 7), 7: (8, 1, 50), 3: (2, 9, 50)}}
    c, g, rep = run(edges, [[0, 2], [7, 3]], [[2], [2]])     # both unique paths are edge 1
    assert (c, g, rep["classes"], rep["lengths"], rep["shared"]) == ([[0, 2], [7, 3]], [[2], [2]], [["shared"], ["shared"]], [[2], [2]], 2)
    c, g, rep = run(edges, [[0, 2], [7, 3]], [[2], [3]])     # the second finds nothing: the first is alone on it
    assert (c, rep["classes"]) == ([[0, 1, 2], [7, 3]], [["filled"], ["none"]])
    c, g, rep = run(edges, [[0, 2], [1]], [[2], []])         # the filler is a member of another chain
    assert (c, rep["classes"], rep["shared"]) == ([[0, 2], [1]], [["shared"], []], 1)
    loop = {**BASE, **{5: (3, 0, 4)}}                      # from the end of 2 to the start of 0 over edge 5: S = 4, L = -1
    c, g, rep = run(loop, [[2, 0]], [[-1]])
    assert (c, rep["classes"]) == ([[2, 5, 0]], [["filled"]])


def test_a_dead_edge_is_no_edge():
    edges = {**BASE, **{10: (1, 11, 4), 11: (11, 2, 4)}}
    assert one(edges, 3)[0] == "filled"
    del edges[11]
    assert one(edges, 3)[0] == "none"


def test_a_displaced_edge_is_on_no_path():
    edges = {**BASE, **{10: (1, 11, 4), 11: (11, 2, 4), 20: (1, 21, 1), 22: (1, 23, 1)}}
    cls, chain, _g, rep = one(edges, 3, max_paths=2)         # four sequences forward, two backward (11, 10 11; 0 is too long)
    assert (cls, chain, rep["searched_backward"]) == ("filled", [0, 10, 11, 2], 1)
    for mp in (2, 256):                                      # found from neither side, and still a member where it is one
        c, g, rep = FR.fill(edges, K, [[0, 2]], [[3]], 0, max_paths=mp, displaced={11})
        assert (c, rep["classes"]) == ([[0, 2]], [["none"]])
    c, g, rep = FR.fill(edges, K, [[0, 2], [11]], [[3], []], 0, displaced={20})
    assert rep["classes"] == [["shared"], []]


def fan(edges, node, first, outward, n=3):
    for i in range(n):
        edges[first + i] = (node, first + i, 1) if outward else (first + i, node, 1)


def test_overflow_takes_both_trees():
    edges = {**BASE, **{1: (1, 2, 7)}}
    fan(edges, 1, 20, True)                                  # four sequences leave node 1 within B = 7
    assert one(edges, 2, max_paths=4)[3]["searched_backward"] == 0
    cls, chain, gaps, rep = one(edges, 2, max_paths=3)       # the forward tree is over, the backward one is edge 1 alone (0 is too long)
    assert (cls, chain, rep["searched_backward"], rep["overflow"]) == ("filled", [0, 1, 2], 1, 0)
    fan(edges, 2, 30, False)                                 # and four sequences reach node 2
    cls, chain, gaps, rep = one(edges, 2, max_paths=3)
    assert (cls, chain, gaps, rep["lengths"], rep["overflow"], rep["searched_backward"]) == ("overflow", [0, 2], [2], [[0]], 1, 1)
    assert one(edges, 2, max_paths=4)[0] == "filled"
    # overflow comes before none and ambiguous
    assert one(edges, 3, max_paths=3)[0] == "overflow" and one(edges, 3, max_paths=4)[0] == "none"


def test_the_mirrored_graph_swaps_the_sides_and_keeps_the_outcome():
    edges = {**BASE, **{1: (1, 2, 7)}}
    fan(edges, 1, 20, True)
    mirrored = {x: (t, s, n) for x, (s, t, n) in edges.items()}
    a = FR.fill(edges, K, [[0, 2]], [[2]], 0, max_paths=3)
    b = FR.fill(mirrored, K, [[2, 0]], [[2]], 0, max_paths=3)
    assert a[0] == [[0, 1, 2]] and b[0] == [[2, 1, 0]] and a[1] == b[1]
    assert (a[2]["searched_backward"], b[2]["searched_backward"]) == (1, 0)
    assert {n: a[2][n] for n in FR.STATS[:9]} == {n: b[2][n] for n in FR.STATS[:9]}


def test_errors():
    edges = {**BASE, **{1: (1, 2, 7)}}
    ok = dict(chains=[[0, 2]], gaps=[[2]], tol=0, max_edges=16, max_paths=256)
    assert FR.check(edges, **ok) is None
    for change in (dict(chains=[[0, 9]]), dict(chains=[[0, 2, 0]], gaps=[[2, 2]]), dict(chains=[[0, 2], []], gaps=[[2], []]), dict(tol=-1), dict(tol=FR.I31 + 1),
                   dict(max_edges=0), dict(max_edges=FR.MAX_EDGES + 1), dict(max_paths=0), dict(max_paths=FR.MAX_PATHS + 1), dict(gaps=[[FR.I31 + 1]]),
                   dict(gaps=[[-FR.I31 - 1]])):
        assert FR.check(edges, **dict(ok, **change)) == "GK_E_INVALID", change
    assert FR.check(edges, [[0, 1, 2]], [[FR.I31 + 1, 0]], 0, 16, 256) is None      # an adjacent junction's gap is not looked at
    assert FR.MAX_PATHS >= 256


@pytest.mark.parametrize("k", [21, 47])
def test_a_chain_and_its_twin_chain_are_filled_alike(k):
    """the oracle's graph is strand-closed: the junction (e, f) and the junction (twin f, twin e), in one call, end in the same
    class, and a filled path is the other's twins reversed"""
    oe = SC.oracle_edges(k, small_pairs(100 + k, k))
    twin = SC.twins(oe)
    edges = {key: (s, e, len(q)) for key, (s, e, q) in oe.items()}
    outs = {}
    for key in sorted(edges):
        outs.setdefault(edges[key][0], []).append(key)
    rnd = random.Random(k)
    seen = {cls: 0 for cls in FR.CLASSES[1:]}
    for trial in range(300):
        e = rnd.choice(sorted(edges))
        walk, at = [], edges[e][1]
        for _ in range(rnd.randint(2, 6)):
            if at not in outs:
                break
            walk.append(rnd.choice(outs[at]))
            at = edges[walk[-1]][1]
        if len(walk) < 2:
            continue
        f, fillers = walk[-1], walk[:-1]
        if len({e, f, twin[e], twin[f]}) < 4:
            continue
        L = sum(edges[x][2] for x in fillers) - k
        for tol, me, mp in ((0, 8, 256), (3, 3, 4), (1, 8, 1)):
            G = L + rnd.choice((-tol - 1, -tol, 0, tol, tol + 1))
            c, g, rep = FR.fill(edges, k, [[e, f], [twin[f], twin[e]]], [[G], [G]], tol, me, mp)
            assert c[1] == [twin[x] for x in reversed(c[0])] and g[1] == g[0][::-1]
            assert rep["classes"][0] == rep["classes"][1] and rep["lengths"][0] == rep["lengths"][1]
            seen[rep["classes"][0][0]] += 1
    assert seen["filled"] > 0 and seen["none"] > 0, seen


def test_the_planted_cases_hold_every_class():
    """what tests/test_fillgaps_gpu.py compares on the device, on the restatement alone: over its graphs and parameters at least
    three junctions of every class, shared by each of its three causes, and junctions decided by the backward tree"""
    seen = dict.fromkeys(FR.CLASSES[1:], 0)
    cause = dict(member=0, other=0, twice=0)
    back = 0
    for k in FC.KS:
        edits, chains, exact, kinds = FC.planted(k)
        edges = FC.apply(FC.base(k), edits)
        assert sorted(x for c in chains for x in c) == sorted({x for c in chains for x in c})
        assert max(sum(1 for v in edges.values() if v[1] == n) for n in {v[1] for v in edges.values()}) > 4
        where = set()
        for tol, mp, me, d in FC.sweep():
            _c, _g, rep = FR.fill(edges, k, chains, FC.gaps(exact, d), tol, me, mp)
            back += rep["searched_backward"] - rep["overflow"]
            for c, cl in enumerate(rep["classes"]):
                for j, name in enumerate(cl):
                    if (c, j, name) not in where:
                        where.add((c, j, name))
                        seen[name] += 1
            if (tol, mp, me, d) == (0, FR.MAX_PATHS, 8, 0):
                for name, kind in (("member", "member"), ("other", "pair"), ("twice", "loop")):
                    cause[name] += sum(rep["classes"][c][j] == "shared" for c, j, _s in kinds[kind])
        # the wide gadget: hundreds of paths from either side with eight edges: over 64, within GK_FILL_MAX_PATHS
        (c, j, _), = kinds[FC.WIDE]
        assert FR.fill(edges, k, chains, FC.gaps(exact, 0), 0, 8, 64)[2]["classes"][c][j] == "overflow"
        assert FR.fill(edges, k, chains, FC.gaps(exact, 0), 0, 8, FR.MAX_PATHS)[2]["classes"][c][j] != "overflow"
        e, f = chains[c]
        outs = {}
        for x, v in edges.items():
            outs.setdefault(v[0], []).append(x)
        tree = FR.sequences(edges, outs, lambda x: edges[x][1], edges[e][1], exact[c][j] + k, 8, FR.MAX_PATHS)
        assert len(tree) > 512 and sum(len(p) == 8 for p, _s in tree) > 64          # a last level of several trips of a wave
    assert min(seen.values()) >= 3 and min(cause.values()) >= 3 and back > 0, (seen, cause, back)
