"""A string-based restatement of the read-threading rule of include/genome_amd.h (gk_graph_thread_reads), for the tests.  It never
touches the device's position map or its graph arrays: a graph is given as node k-mers (one entry per node, so the copies of a
split node repeat) and edges (start node index, end node index, sequence); positions follow insert_ref.index_graph's
convention: ("N", node index) or ("E", edge index, distance)."""
from collections import Counter

from insert_ref import index_graph
from oracle import pyref as R

STATS = ("records", "inner_windows", "off_graph", "repeated", "on_edge", "broken", "crossings")


def thread_reads(k, nodes, edges, reads):
    """-> (Counter {(in-edge index, out-edge index): crossings}, {stat: count})"""
    index, lens = index_graph(k, [(nodes[s], q) for s, _, q in edges], nodes=nodes)
    out_edge = {}
    for e, (s, _, q) in enumerate(edges):
        assert (s, q[0]) not in out_edge, "two out-edges of one node share a first base"
        out_edge[(s, q[0])] = e
    end = [t for _, t, _ in edges]
    sup, st = Counter(), dict.fromkeys(STATS, 0)
    for r in reads:
        L = len(r)
        if L < k + 2:
            continue
        st["records"] += 1
        for s in (r, R.rev_comp(r)):
            P = [index.get(s[i:i + k], []) for i in range(L - k + 1)]
            for i in range(1, L - k):
                st["inner_windows"] += 1
                if not P[i]:
                    st["off_graph"] += 1
                elif len(P[i]) >= 2:
                    st["repeated"] += 1
                elif P[i][0][0] == "E":
                    st["on_edge"] += 1
                else:
                    v = P[i][0][1]
                    f = out_edge.get((v, s[i + k]))
                    exit_ok = f is not None and len(P[i + 1]) == 1 and P[i + 1][0] == (("E", f, 1) if lens[f] > 1 else ("N", end[f]))
                    e = None
                    if len(P[i - 1]) == 1:
                        p = P[i - 1][0]
                        if p[0] == "E":
                            if p[2] == lens[p[1]] - 1 and end[p[1]] == v:
                                e = p[1]
                        else:
                            c = out_edge.get((p[1], s[i + k - 1]))
                            if c is not None and lens[c] == 1 and end[c] == v:
                                e = c
                    if exit_ok and e is not None:
                        st["crossings"] += 1
                        sup[(e, f)] += 1
                    else:
                        st["broken"] += 1
    return sup, st


def twin_edges(k, nodes, edges):
    """edge index -> the index of its reverse-complement twin (a strand-closed graph without node copies); KeyError if one has none"""
    by_path = {nodes[s] + q: e for e, (s, _, q) in enumerate(edges)}
    return {e: by_path[R.rev_comp(nodes[s] + q)] for e, (s, _, q) in enumerate(edges)}
