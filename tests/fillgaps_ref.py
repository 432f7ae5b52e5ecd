"""A restatement of the gap-filling rule (include/genome_amd.h, "gap filling") by plain recursion and set sizes: no levels, no
tree in a fixed store, no strands.

fill(edges, k, ...) takes the live edges as {edge id: (start node, end node, len)}; nodes and ids are anything hashable, two
edges meet iff one's end == the other's start.  Chains are lists of edge ids, gaps[c][i] the gap after member i of chain c, as
scaffolds_ref takes them.  -> (chains, gaps, report) in the shape of HipGraph.fillGaps.  `displaced`: live edges that their start
node's out-edge word no longer names (gk_graph_replace_start put another edge of the same first base there): they are on no path,
from either side, and are edges in every other respect.
"""
STATS = ("junctions", "adjacent", "overflow", "none", "ambiguous", "shared", "filled", "filler_edges", "filler_bases", "searched_backward")
CLASSES = ("last", "adjacent", "overflow", "none", "ambiguous", "shared", "filled")
MAX_EDGES, MAX_PATHS = 64, 1024
I31 = 2 ** 31 - 1


class TooMany(Exception):
    pass


def sequences(edges, step, far, root, B, max_edges, max_paths):
    """every sequence of 1..max_edges edges with sum <= B that starts in `root`, where step[node] lists the edges that leave it
    in this direction and far(edge) is the node an edge leads to; TooMany as soon as there are more than max_paths"""
    found = []

    def grow(node, seq, total):
        for x in step.get(node, ()):
            if total + edges[x][2] > B:
                continue
            found.append((seq + [x], total + edges[x][2]))
            if len(found) > max_paths:
                raise TooMany
            if len(seq) + 1 < max_edges:
                grow(far(x), seq + [x], total + edges[x][2])

    grow(root, [], 0)
    return found


def junction(edges, outs, ins, k, e, f, G, tol, max_edges, max_paths):
    """-> (class or 'unique', path, L, searched backward)"""
    if edges[e][1] == edges[f][0]:
        return "adjacent", None, 0, False
    B = G + tol + k
    if B < 1:
        return "none", None, 0, False
    back = False
    try:
        hits = [(p, s) for p, s in sequences(edges, outs, lambda x: edges[x][1], edges[e][1], B, max_edges, max_paths) if edges[p[-1]][1] == edges[f][0]]
    except TooMany:
        back = True
        try:
            hits = [(p[::-1], s) for p, s in sequences(edges, ins, lambda x: edges[x][0], edges[f][0], B, max_edges, max_paths) if edges[p[-1]][0] == edges[e][1]]
        except TooMany:
            return "overflow", None, 0, True
    hits = [(p, s - k) for p, s in hits if G - tol <= s - k <= G + tol]
    if not hits:
        return "none", None, 0, back
    if len(hits) > 1:
        return "ambiguous", None, 0, back
    return "unique", hits[0][0], hits[0][1], back


def check(edges, chains, gaps, tol, max_edges, max_paths):
    """None, or the name of the error the input has"""
    if not 0 <= tol <= I31 or not 1 <= max_edges <= MAX_EDGES or not 1 <= max_paths <= MAX_PATHS:
        return "GK_E_INVALID"
    seen = set()
    for c in chains:
        if not c:
            return "GK_E_INVALID"
        for e in c:
            if e not in edges or e in seen:
                return "GK_E_INVALID"
            seen.add(e)
    for c, g in zip(chains, gaps):
        for e, f, G in zip(c, c[1:], g):
            if edges[e][1] != edges[f][0] and abs(G) > I31:
                return "GK_E_INVALID"
    return None


def fill(edges, k, chains, gaps, tol, max_edges=16, max_paths=256, displaced=()):
    assert check(edges, chains, gaps, tol, max_edges, max_paths) is None
    outs, ins = {}, {}
    for x, (s, t, _n) in edges.items():
        if x in displaced:
            continue
        outs.setdefault(s, []).append(x)
        ins.setdefault(t, []).append(x)
    st = dict.fromkeys(STATS, 0)
    found = [[junction(edges, outs, ins, k, e, f, G, tol, max_edges, max_paths) for e, f, G in zip(c, c[1:], g)] for c, g in zip(chains, gaps)]
    uses = {}
    for c in chains:
        for e in c:
            uses[e] = uses.get(e, 0) + 2                    # a member is contested by any use
    for js in found:
        for cls, path, _L, _b in js:
            if cls == "unique":
                for x in path:
                    uses[x] = uses.get(x, 0) + 1
    out_chains, out_gaps, classes, lengths = [], [], [], []
    for c, g, js in zip(chains, gaps, found):
        oc, og, cl, ln = [c[0]], [], [], []
        for f, G, (cls, path, L, back) in zip(c[1:], g, js):
            st["searched_backward"] += back
            if cls == "unique":
                cls = "shared" if any(uses[x] > 1 for x in path) else "filled"
                ln.append(L)
            else:
                ln.append(0)
            if cls == "filled":
                oc += path
                og += [-k] * (len(path) + 1)
                st["filler_edges"] += len(path)
                st["filler_bases"] += L + k
            else:
                og.append(G)
            oc.append(f)
            st[cls] += 1
            st["junctions"] += 1
            cl.append(cls)
        out_chains.append(oc); out_gaps.append(og); classes.append(cl); lengths.append(ln)
    report = dict(st, classes=classes, lengths=lengths)
    return out_chains, out_gaps, report
