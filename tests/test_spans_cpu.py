"""The restatement of the span rules (tests/spans_ref.py) against hand-made graphs whose answers are known by construction.  No GPU."""
import random
from collections import Counter

import pytest

from oracle import pyref as R
from spans_ref import split_edges, thread_spans
from thread_ref import thread_reads, twin_edges

K = 5


def valid(paths):
    """a graph as a build would leave it, on both strands: every node k-mer and every interior window of an edge occurs once, and
    the out-edges of a node start with different bases"""
    paths = list(paths) + [R.rev_comp(p) for p in paths]
    nodes = {p[:K] for p in paths} | {p[-K:] for p in paths}
    kmers = list(nodes) + [p[d:d + K] for p in paths for d in range(1, len(p) - K)]
    return len(set(kmers)) == len(kmers) and len({p[:K + 1] for p in paths}) == len(paths)


def strings(seed, lens, paths=lambda *pieces: pieces):
    """random strings of the given lengths, from the first seed at which the paths made of them are a valid graph"""
    for s in range(seed, seed + 10000):
        rnd = random.Random(s)
        out = ["".join(rnd.choice("AGCT") for _ in range(n)) for n in lens]
        if valid(paths(*out)):
            return out
    raise AssertionError("no seed")


def graph(paths, both_strands=False):
    """paths (start k-mer ++ sequence) -> (nodes, edges) as thread_ref takes them; edge e is paths[e] (then its reverse complement)"""
    if both_strands:
        paths = list(paths) + [R.rev_comp(p) for p in paths]
    nodes = sorted({p[:K] for p in paths} | {p[-K:] for p in paths})
    return nodes, [(nodes.index(p[:K]), nodes.index(p[-K:]), p[K:]) for p in paths]


def fork(r, flank=8, seed=1):
    """two ways in (edges 0, 1), a repeat of r bases (edge 2, r - K long), two ways out (edges 3, 4) -> (pieces, nodes, edges)"""
    paths = lambda A1, A2, Rp, B1, B2: [A1 + Rp[:K], A2 + Rp[:K], Rp, Rp[-K:] + B1, Rp[-K:] + B2]
    pieces = strings(seed, [flank, flank, r, flank, flank], paths)
    return pieces, *graph(paths(*pieces))


def test_a_straight_read_over_a_repeat_is_one_span():
    (A1, A2, Rp, B1, B2), nodes, edges = fork(K + 4)
    spans, st = thread_spans(K, nodes, edges, [A1 + Rp + B1, A2 + Rp + B2, A2 + Rp + B2])
    assert spans == Counter({(0, 2, 3): 1, (1, 2, 4): 2})
    # per read: the crossing into the repeat is open (the read began on the flank), the one out of it is the span
    assert st == {"records": 3, "crossings": 6, "spans": 3, "interrupted": 0, "open": 3}
    assert st["crossings"] == thread_reads(K, nodes, edges, [A1 + Rp + B1, A2 + Rp + B2, A2 + Rp + B2])[1]["crossings"]


def test_edges_of_length_one_on_both_sides():
    """a repeat of K + 1 bases is an edge of length 1: the window before the second crossing is the first one, a node; with flanks
    of one base the in- and out-edge have length 1 too and the crossings are recognised through node positions alone"""
    x1, x2, y1, y2 = "ACGT"
    paths = lambda Rp: [x1 + Rp[:K], x2 + Rp[:K], Rp, Rp[-K:] + y1, Rp[-K:] + y2]
    Rp, = strings(3, [K + 1], paths)
    nodes, edges = graph(paths(Rp))
    assert [len(q) for _, _, q in edges] == [1] * 5
    spans, st = thread_spans(K, nodes, edges, [x1 + Rp + y1, x2 + Rp + y2])
    assert spans == Counter({(0, 2, 3): 1, (1, 2, 4): 1})
    assert st == {"records": 2, "crossings": 4, "spans": 2, "interrupted": 0, "open": 2}


def test_a_read_that_starts_inside_the_repeat_is_open():
    (A1, A2, Rp, B1, B2), nodes, edges = fork(K + 6)
    for start in (0, 1, 3):            # at the start node, and inside
        spans, st = thread_spans(K, nodes, edges, [Rp[start:] + B1])
        assert not spans and st == {"records": 1, "crossings": 1, "spans": 0, "interrupted": 0, "open": 1}


def test_a_wrong_base_inside_the_repeat_interrupts():
    """r = 2K + 3: base K + 1 of the repeat lies in the windows at distances 2 .. K + 1 of the edge (8 long) and in neither crossing
    nor in the windows next to them, so both crossings stand and only the walk between them fails"""
    (A1, A2, Rp, B1, B2), nodes, edges = fork(2 * K + 3)
    bad = Rp[:K + 1] + ("A" if Rp[K + 1] != "A" else "C") + Rp[K + 2:]
    spans, st = thread_spans(K, nodes, edges, [A1 + bad + B1])
    assert not spans and st == {"records": 1, "crossings": 2, "spans": 0, "interrupted": 1, "open": 1}
    assert thread_reads(K, nodes, edges, [A1 + bad + B1])[1]["crossings"] == 2
    # a wrong base in the first crossing's own window: no crossing there, the second is interrupted as well
    bad = Rp[:1] + ("A" if Rp[1] != "A" else "C") + Rp[2:]
    assert thread_spans(K, nodes, edges, [A1 + bad + B1])[1] == {"records": 1, "crossings": 1, "spans": 0, "interrupted": 1, "open": 0}


def test_three_nodes_in_a_row_are_two_spans():
    paths = lambda A, M1, M2, B: [A + M1[:K], M1, M1[-K:] + M2, M2[-K:] + B]
    A, M1, M2, B = strings(5, [8, K + 2, K + 1, 8], paths)
    nodes, edges = graph(paths(A, M1, M2, B))
    # edges: 0 = A into u, 1 = u..w (2 long), 2 = w..v (K + 1 long), 3 = v onwards
    spans, st = thread_spans(K, nodes, edges, [A + M1 + M2 + B])
    assert spans == Counter({(0, 1, 2): 1, (1, 2, 3): 1})
    assert st == {"records": 1, "crossings": 3, "spans": 2, "interrupted": 0, "open": 1}


def test_twin_triples():
    (A1, A2, Rp, B1, B2), nodes, edges = fork(K + 3, seed=7)
    nodes, edges = graph([nodes[s] + q for s, _, q in edges], both_strands=True)
    tw = twin_edges(K, nodes, edges)
    reads = [A1 + Rp + B1, R.rev_comp(A2 + Rp + B2), A1 + Rp + B2, (A2 + Rp + B1)[3:-2]]
    spans, st = thread_spans(K, nodes, edges, reads)
    assert st["spans"] == 8 and len(spans) == 8
    for (e, m, f), c in spans.items():
        assert spans[(tw[f], tw[m], tw[e])] == c


def arbrc(seed=11, r=K + 4):
    paths = lambda A, Rp, B, C: [A + Rp[:K], Rp, Rp[-K:] + B + Rp[:K], Rp[-K:] + C]
    A, Rp, B, C = strings(seed, [8, r, 9, 8], paths)
    nodes, edges = graph(paths(A, Rp, B, C))
    return A + Rp + B + Rp + C, nodes, edges


def spell(nodes, edges, start_edge):
    """the sequence of the unbranched path from an edge on"""
    outs = {}
    for e, x in enumerate(edges):
        if x is not None:
            outs.setdefault(x[0], []).append(e)
    e, s, seen = start_edge, nodes[edges[start_edge][0]], set()
    while e is not None and e not in seen:
        seen.add(e)
        s += edges[e][2]
        nxt = outs.get(edges[e][1], [])
        e = nxt[0] if len(nxt) == 1 else None
    return s


def test_split_of_a_r_b_r_c_gives_one_path():
    g, nodes, edges = arbrc()
    L = 2 * K + len(edges[1][2]) + 2
    spans, st = thread_spans(K, nodes, edges, [g[i:i + L] for i in range(len(g) - L + 1)])
    assert set(spans) == {(0, 1, 2), (2, 1, 3)} and st["interrupted"] == 0
    n2, e2, st2 = split_edges(nodes, edges, spans, 1)
    assert st2 == {"candidates": 1, "resolved": 1, "unequal": 0, "ambiguous": 0, "unsupported": 0, "new_edges": 1, "new_nodes": 2}
    u, v = edges[1][0], edges[1][1]
    # A keeps u, m and v; B now ends at u' and C starts at v', which the copy of m joins
    assert n2[len(nodes):] == [nodes[u], nodes[v]] and e2[4] == (len(nodes), len(nodes) + 1, edges[1][2])
    assert e2[0] == edges[0] and e2[1] == edges[1] and e2[2] == (v, len(nodes), edges[2][2]) and e2[3] == (len(nodes) + 1, edges[3][1], edges[3][2])
    assert spell(n2, e2, 0) == g
    # a second call with the same, now stale, table finds nothing left to do
    assert split_edges(n2, e2, spans, 1)[2]["candidates"] == 0


def square(p, q):
    """p ways in (edges 0 .. p-1), the repeat (edge p), q ways out (edges p+1 ..)"""
    paths = lambda *x: [a + x[p][:K] for a in x[:p]] + [x[p]] + [x[p][-K:] + b for b in x[p + 1:]]
    return graph(paths(*strings(13, [8] * p + [K + 3] + [8] * q, paths)))


@pytest.mark.parametrize("spans, cls", [
    ({(0, 2, 3): 5, (1, 2, 4): 5}, "resolved"),
    ({(0, 2, 4): 5, (1, 2, 3): 5}, "resolved"),
    ({(0, 2, 3): 5, (1, 2, 4): 5, (0, 2, 4): 5}, "ambiguous"),
    ({(0, 2, 3): 5, (1, 2, 3): 5}, "ambiguous"),            # ambiguous is tested before unsupported
    ({(0, 2, 3): 5}, "unsupported"),
    ({}, "unsupported"),
    ({(0, 2, 3): 5, (1, 2, 4): 4}, "unsupported"),          # one below the cutoff
    ({(0, 2, 3): 5, (1, 2, 4): 5, (0, 2, 4): 4, (7, 2, 3): 9, (0, 9, 3): 9}, "resolved"),   # below the cutoff, and names nothing here
])
def test_the_classes_of_a_candidate(spans, cls):
    nodes, edges = square(2, 2)
    n2, e2, st = split_edges(nodes, edges, spans, 5)
    assert st["candidates"] == 1 and st[cls] == 1 and st["new_edges"] == (1 if cls == "resolved" else 0)
    if cls != "resolved":
        assert (n2, e2) == (nodes, edges)
    else:
        j = 4 if spans.get((1, 2, 4), 0) >= 5 else 3
        assert e2[1][1] == len(nodes) and e2[j][0] == len(nodes) + 1 and e2[5] == (len(nodes), len(nodes) + 1, edges[2][2])


def test_unequal_and_non_candidates():
    nodes, edges = square(3, 2)
    n2, e2, st = split_edges(nodes, edges, {(0, 3, 4): 9, (1, 3, 5): 9}, 1)
    assert st["candidates"] == 1 and st["unequal"] == 1 and (n2, e2) == (nodes, edges)
    nodes, edges = square(1, 2)                              # one way in: the node split's business
    assert split_edges(nodes, edges, {(0, 1, 2): 9}, 1)[2]["candidates"] == 0
    nodes, edges = square(3, 3)
    perm = {(0, 3, 6): 2, (1, 3, 4): 2, (2, 3, 5): 2}
    n2, e2, st = split_edges(nodes, edges, perm, 2)
    assert st["resolved"] == 1 and st["new_edges"] == 2 and st["new_nodes"] == 4
    # ids in order of a_i: edge 1's pair gets nodes n, n+1 and edge 7; edge 2's pair nodes n+2, n+3 and edge 8
    n = len(nodes)
    assert (e2[1][1], e2[4][0], e2[7][:2]) == (n, n + 1, (n, n + 1)) and (e2[2][1], e2[5][0], e2[8][:2]) == (n + 2, n + 3, (n + 2, n + 3))
    assert e2[0] == edges[0] and e2[6] == edges[6]
    assert split_edges(nodes, edges, perm, 3)[2]["unsupported"] == 1
