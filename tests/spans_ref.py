"""A string-based restatement of the two span rules of include/genome_amd.h (gk_graph_thread_spans, gk_graph_split_edges_by_spans),
for the tests.  It never touches device arrays: a graph is given as thread_ref.thread_reads takes it, node k-mers (one entry per
node, so copies repeat) and edges (start node index, end node index, sequence), and positions follow insert_ref.index_graph's
convention.  The window classes are thread_ref.thread_reads', row for row (test_spans_cpu.py holds the two to each other)."""
from collections import Counter

from insert_ref import index_graph
from oracle import pyref as R

STATS = ("records", "crossings", "spans", "interrupted", "open")
SPLIT_STATS = ("candidates", "resolved", "unequal", "ambiguous", "unsupported", "new_edges", "new_nodes")


def crossings(k, index, lens, out_edge, end, s):
    """{inner window i of strand s: (e, f)} for the windows whose class is `crossing`"""
    L = len(s)
    P = [index.get(s[i:i + k], []) for i in range(L - k + 1)]
    X = {}
    for i in range(1, L - k):
        if len(P[i]) != 1 or P[i][0][0] != "N":
            continue
        v = P[i][0][1]
        f = out_edge.get((v, s[i + k]))
        if f is None or len(P[i + 1]) != 1 or P[i + 1][0] != (("E", f, 1) if lens[f] > 1 else ("N", end[f])):
            continue
        if len(P[i - 1]) != 1:
            continue
        p = P[i - 1][0]
        if p[0] == "E":
            e = p[1] if p[2] == lens[p[1]] - 1 and end[p[1]] == v else None
        else:
            e = out_edge.get((p[1], s[i + k - 1]))
            if e is not None and not (lens[e] == 1 and end[e] == v):
                e = None
        if e is not None:
            X[i] = (e, f)
    return X, P


def thread_spans(k, nodes, edges, reads):
    """-> (Counter {(in-edge index, spanned edge index, out-edge index): reads}, {stat: count})"""
    index, lens = index_graph(k, [(nodes[s], q) for s, _, q in edges], nodes=nodes)
    out_edge = {(s, q[0]): e for e, (s, _, q) in enumerate(edges)}
    end = [t for _, t, _ in edges]
    spans, st = Counter(), dict.fromkeys(STATS, 0)
    for r in reads:
        if len(r) < k + 2:
            continue
        st["records"] += 1
        for s in (r, R.rev_comp(r)):
            X, P = crossings(k, index, lens, out_edge, end, s)
            for j, (m, f) in sorted(X.items()):
                st["crossings"] += 1
                i = j - lens[m]
                if i < 1:
                    st["open"] += 1
                elif i in X and X[i][1] == m and all(P[t] == [("E", m, t - i)] for t in range(i + 1, j)):
                    st["spans"] += 1
                    spans[(X[i][0], m, f)] += 1
                else:
                    st["interrupted"] += 1
    return spans, st


def split_edges(nodes, edges, spans, cutoff):
    """nodes: the list of node k-mers by id (None = a dead id); edges: by id, (start id, end id, sequence) or None; spans: {(e, m,
    f): count} by id -> (new nodes, new edges in id order, {stat: count}).  Triples that name nothing here are never looked up."""
    assert cutoff >= 1
    nodes, new_edges = list(nodes), list(edges)
    ins, outs = {}, {}
    for e, x in enumerate(edges):
        if x is not None:
            outs.setdefault(x[0], []).append(e)
            ins.setdefault(x[1], []).append(e)
    st = dict.fromkeys(SPLIT_STATS, 0)
    for m, x in enumerate(edges):
        if x is None:
            continue
        u, v, seq = x
        a, b = sorted(ins.get(u, [])), sorted(outs.get(v, []))
        if len(outs[u]) != 1 or len(ins[v]) != 1 or len(a) < 2 or len(b) < 2:
            continue
        st["candidates"] += 1
        if len(a) != len(b):
            st["unequal"] += 1
            continue
        M = [[spans.get((ai, m, bj), 0) >= cutoff for bj in b] for ai in a]
        lines = [sum(row) for row in M] + [sum(col) for col in zip(*M)]
        if max(lines) >= 2:
            st["ambiguous"] += 1
            continue
        if min(lines) == 0:
            st["unsupported"] += 1
            continue
        st["resolved"] += 1
        for i in range(1, len(a)):
            j = M[i].index(True)
            nu, nv = len(nodes), len(nodes) + 1
            nodes += [nodes[u], nodes[v]]
            new_edges.append((nu, nv, seq))
            # (decided on the graph as it was: an edge may be moved at its end by one pair and at its start by another)
            s0, _, q0 = new_edges[a[i]]
            new_edges[a[i]] = (s0, nu, q0)
            _, t0, q0 = new_edges[b[j]]
            new_edges[b[j]] = (nv, t0, q0)
            st["new_edges"] += 1
            st["new_nodes"] += 2
    return nodes, new_edges, st
