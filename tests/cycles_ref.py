"""Plain-Python restatement of the two "perfect cycles" rules (include/genome_amd.h), independent of the device code: strings,
sets and dicts only.

k-mer level.  `table` is the set of stored k-mers (either strand of each); `present` = table and its reverse complements.
An oriented k-mer is a member iff it has one successor and one predecessor and following successors never reaches a terminal
k-mer.  Members form cycles; the anchors of a cycle are its members with the smallest anchor key; every anchor gets one edge,
the arc to the next anchor.

node level.  The keeping simplify on a graph in canonical form (node strings, edges (start, end, seq)).
"""
from genome_amd import dna

BASES = dna.BASES


def rc(s):
    return dna.rev_complement(s)


def anchor_key(s):
    """min(x, rc x) as 2-bit-packed integers compared as (hi, lo)"""
    a, b = dna.pack(s), dna.pack(rc(s))
    return min((a[1], a[0]), (b[1], b[0]))


def _order(s):
    lo, hi = dna.pack(s)
    return (hi, lo)


def circular_kmers(c, k):
    """the k-mers of the circular sequence c, in order (len(c) of them; c may be shorter than k)"""
    ext = (c * (k // len(c) + 2))[:len(c) + k - 1]
    return [ext[i:i + k] for i in range(len(c))]


def linear_kmers(s, k):
    return [s[i:i + k] for i in range(len(s) - k + 1)]


def oriented(table):
    return set(table) | {rc(x) for x in table}


def degrees(present, u):
    succ = [u[1:] + b for b in BASES if u[1:] + b in present]
    pred = [b + u[:-1] for b in BASES if b + u[:-1] in present]
    return pred, succ


def is_terminal(present, u):
    pred, succ = degrees(present, u)
    ni, no = len(pred), len(succ)
    return (ni != 1 or no != 1) and (ni != 0 or no != 0)          # Graph.scala:323


def cycles(present):
    """-> the oriented cycles of members, each a list of k-mers in successor order (rotation unspecified)"""
    state = {}                                                      # k-mer -> True (member) / False
    out = []
    for u0 in sorted(present):
        if u0 in state:
            continue
        path, on_path, u, verdict = [], set(), u0, None
        while verdict is None:
            if u in state:
                verdict = state[u]
                break
            pred, succ = degrees(present, u)
            if len(pred) != 1 or len(succ) != 1:
                # terminal, or (0, 0): what came before it on the path leaves the set of candidates
                state[u] = False
                verdict = False
                break
            if u in on_path:
                verdict = True                                      # back on the path: predecessors are unique, so u == u0
                assert u == u0
                break
            path.append(u)
            on_path.add(u)
            u = succ[0]
        for x in path:
            state[x] = verdict
        if verdict and path and path[0] == u:
            out.append(path)
    return out


def build_edit(table):
    """-> (nodes added, edges added as (start, end, seq), stats dict) of gk_graph_build_cycles on this table"""
    present = oriented(table)
    cyc = cycles(present)
    nodes, edges = [], []
    two = selfc = longest = 0
    for c in cyc:
        best = min(anchor_key(u) for u in c)
        at = [i for i, u in enumerate(c) if anchor_key(u) == best]
        assert len(at) in (1, 2)
        two += len(at) == 2
        selfc += {rc(u) for u in c} == set(c)
        longest = max(longest, len(c))
        for j, i in enumerate(at):
            nxt = at[(j + 1) % len(at)]
            steps = (nxt - i) % len(c) or len(c)
            seq = "".join(c[(i + s) % len(c)][-1] for s in range(1, steps + 1))
            nodes.append(c[i])
            edges.append((c[i], c[nxt], seq))
    members = sum(len(c) for c in cyc)
    rounds = 0
    while (1 << rounds) < members:
        rounds += 1
    stats = {"cycle_kmers": members, "cycles": len(cyc), "anchors": len(nodes), "self_complementary": selfc, "longest": longest,
             "rounds": rounds}
    assert sum(len(e[2]) for e in edges) == members and len(nodes) == len(cyc) + two
    return nodes, edges, stats


def canonical(nodes, edges):
    """the order of HipGraph.canonical(): nodes by k-mer, edges by (start k-mer, first base)"""
    return (sorted(nodes, key=_order),
            sorted(edges, key=lambda e: (_order(e[0]), BASES.index(e[2][0]))))


def merged(plain, edit):
    return canonical(list(plain[0]) + list(edit[0]), list(plain[1]) + list(edit[1]))


def path_of(edge):
    """start k-mer ++ seq"""
    return edge[0] + edge[2]


def simplify_keep(nodes, edges):
    """-> ((nodes, edges) canonical, stats dict) of gk_graph_simplify_keep_cycles on a canonical graph"""
    out_e, in_e = {n: [] for n in nodes}, {n: [] for n in nodes}
    for i, e in enumerate(edges):
        out_e[e[0]].append(i)
        in_e[e[1]].append(i)
    cls = {}
    for n in nodes:
        ni, no = len(in_e[n]), len(out_e[n])
        if ni == 0 and no == 0:
            cls[n] = 3
        elif ni == 1 and no == 1:
            cls[n] = 2 if in_e[n][0] == out_e[n][0] else 1
        else:
            cls[n] = 0
    stats = {"kept_self_loops": 0, "cycles_merged": 0, "anchors_kept": 0, "nodes_removed": 0}
    for n in nodes:
        if cls[n] == 2:
            cls[n] = 0
            stats["kept_self_loops"] += 1
    succ = {n: edges[out_e[n][0]][1] for n in nodes if cls[n] == 1}
    seen = set()
    for n0 in sorted(succ, key=_order):
        if n0 in seen:
            continue
        path, u = [], n0
        while u in succ and u not in seen:
            seen.add(u)
            path.append(u)
            u = succ[u]
        if u != n0 or u not in succ:
            continue                                                # a chain that ends outside, or runs into one seen before
        if any(succ[x] not in path for x in path):
            continue
        best = min(anchor_key(x) for x in path)
        anchors = [x for x in path if anchor_key(x) == best]
        assert len(anchors) in (1, 2)
        for x in anchors:
            cls[x] = 0
        stats["anchors_kept"] += len(anchors)
        stats["cycles_merged"] += len(anchors) < len(path)
    new_edges, dead = [], set()
    for i, e in enumerate(edges):
        if cls[e[0]] != 0 or cls[e[1]] != 1:
            continue
        seq, cur = "", i
        while True:
            seq += edges[cur][2]
            dead.add(cur)
            v = edges[cur][1]
            if cls[v] != 1:
                break
            cur = out_e[v][0]
        new_edges.append((e[0], v, seq))
    keep_nodes = [n for n in nodes if cls[n] == 0]
    keep_edges = [e for i, e in enumerate(edges) if i not in dead and cls[e[0]] == 0 and cls[e[1]] == 0] + new_edges
    stats["nodes_removed"] = len(nodes) - len(keep_nodes)
    return canonical(keep_nodes, keep_edges), stats
