"""What the gap-filling tests share: a model of the oracle's graph of insert_cases.small_pairs by content, a fixed list of
point edits that plant what the unedited graph lacks (it is nearly a tree: no two paths between two nodes, no cycle, trees of at
most seven paths), and the chains over the edited model.  Content only: an edge is its (start k-mer, first base), a node its
k-mer or ("new", i) for an added one; a GPU test maps both to the device's ids and applies the same edits there.

Every gadget takes the next unused edges of a fixed order, long ones (over 60 bases) as the contigs e and f, short ones as
fillers, and moves their ends onto added nodes, which have no out-edge yet: no out-edge word is ever displaced, and two edges
that leave one added node are chosen with different first bases.
    fan     e -> N0 -x-> N1 -> f, and z leaves N0 for elsewhere: filled; forward over max_paths = 1, backward not
    bubble  e -> N0 -(p | q)-> N1 -> f: ambiguous when the tolerance covers both lengths
    loop    e -> N0 -p-> N0 -y-> N1 -> f, the gap that of p p y: unique, and shared because p occurs twice
    pair    e1, e2 -> N0 -x-> N1 -> f1, f2: two unique paths over x, both shared
    member  e -> N0 -x-> N1 -> f with x a chain of its own: shared
    line    e -> N0 -x1-> .. -xm-> N1 -> f, m = 5 for the first and 3 after it: filled from m edges up
    wide    e -> N0 -(p | q)-> N0 -y-> N1 -> f, once per graph, the gap that of eight times the longer loop and y: with
            max_edges = 8 the trees hold over 512 paths and their last level several trips of a wave; over max_paths = 64 from both sides
and the ends of four more edges go to the first pair's N0 (the first line's where no pair fits), whose in-list then holds six
(five).
"""
import scaffolds_cases as SC
from insert_cases import small_pairs

KINDS = ("fan", "bubble", "loop", "pair", "member", "line")
WIDE = "wide"
KS = (21, 31, 47)
D = lambda tol: (-tol - 1, -tol, 0, tol, tol + 1)


def sweep():
    """(tol, max_paths, max_edges, d): every gap of the planted junctions is the path's L + d"""
    return [(tol, mp, me, d) for tol in (0, 3, 12) for mp in (1, 4, 64, 1024) for me in (1, 3, 8) for d in D(tol)]


def base(k):
    oe = SC.oracle_edges(k, small_pairs(100 + k, k))
    return {key: (s, e, len(q)) for key, (s, e, q) in oe.items()}


def apply(edges, edits):
    """the model after the edits: ("end", key, node), ("start", key, node), ("remove", key); ("node", i) adds ("new", i)"""
    edges = {key: list(v) for key, v in edges.items()}
    for op, *a in edits:
        if op == "end":
            edges[a[0]][1] = a[1]
        elif op == "start":
            edges[a[0]][0] = a[1]
        elif op == "remove":
            del edges[a[0]]
    return {key: tuple(v) for key, v in edges.items()}


def planted(k):
    """-> (edits, chains, exact, kinds): chains of content keys (every edge once); exact[c][i] = the planted path's L at a planted
    junction (the bubble's: the middle of its two), a fixed gap elsewhere; kinds[name] = [(chain, junction, spread)], spread =
    the tolerance from which a bubble is ambiguous and below which a loop's hit is the only one"""
    edges = base(k)
    order = sorted(edges)
    longs = [x for x in order if edges[x][2] > 60]
    shorts = [x for x in order if edges[x][2] <= 60]
    edits, chains, exact, kinds, nodes = [], [], [], {n: [] for n in KINDS}, [0]

    def node():
        nodes[0] += 1
        edits.append(("node", nodes[0] - 1))
        return ("new", nodes[0] - 1)

    def short(n, distinct=False):
        got = []
        for x in list(shorts):
            if len(got) < n and not (distinct and any(x[1] == y[1] for y in got)):
                got.append(x)
                shorts.remove(x)
        return got if len(got) == n else None

    def wire(x, s, t):
        if s is not None:
            edits.append(("start", x, s))
        if t is not None:
            edits.append(("end", x, t))

    # two pairs that meet in a node as they are
    for e in list(shorts):
        near = [f for f in shorts if f != e and edges[f][0] == edges[e][1]]
        if e in shorts and near and len(chains) < 2:
            shorts.remove(e); shorts.remove(near[0])
            chains.append([e, near[0]]); exact.append([25])
    kinds[WIDE] = []
    xs = short(3, distinct=True)
    if len(longs) >= 2 and xs:
        e, f = longs.pop(0), longs.pop(0)
        n0, n1 = node(), node()
        wire(e, None, n0); wire(xs[0], n0, n0); wire(xs[1], n0, n0); wire(xs[2], n0, n1); wire(f, n1, None)
        chains.append([e, f]); exact.append([8 * max(edges[xs[0]][2], edges[xs[1]][2]) + edges[xs[2]][2] - k])
        kinds[WIDE].append((len(chains) - 1, 0, tuple(edges[x][2] for x in xs)))
    hub = line0 = None
    for rnd in range(3):
        for kind in KINDS:
            need_long, need_short = (4, 1) if kind == "pair" else (2, {"fan": 2, "bubble": 2, "loop": 2, "member": 1, "line": 3 if kinds["line"] else 5}[kind])
            if len(longs) < need_long or len(shorts) < need_short + 4:
                continue
            xs = short(need_short, distinct=kind != "line")
            if xs is None:
                continue
            es = [longs.pop(0) for _ in range(need_long)]
            n0, n1 = node(), node()
            L = [edges[x][2] for x in xs]
            if kind == "pair":
                e1, e2, f1, f2 = es
                if f1[1] == f2[1]:                           # two out-edges of N1 need two first bases
                    longs[:0] = es; shorts[:0] = xs
                    continue
                wire(e1, None, n0); wire(e2, None, n0); wire(xs[0], n0, n1); wire(f1, n1, None); wire(f2, n1, None)
                chains += [[e1, f1], [e2, f2]]; exact += [[L[0] - k], [L[0] - k]]
                kinds[kind] += [(len(chains) - 2, 0, 0), (len(chains) - 1, 0, 0)]
                hub = hub or n0
                continue
            e, f = es
            wire(e, None, n0)
            if kind == "fan":
                wire(xs[0], n0, n1); wire(xs[1], n0, None); gap, spread = L[0] - k, 0
            elif kind == "bubble":
                wire(xs[0], n0, n1); wire(xs[1], n0, n1); gap, spread = (L[0] + L[1]) // 2 - k, (abs(L[0] - L[1]) + 1) // 2
            elif kind == "loop":
                wire(xs[0], n0, n0); wire(xs[1], n0, n1); gap, spread = 2 * L[0] + L[1] - k, L[0]
            elif kind == "member":
                wire(xs[0], n0, n1); gap, spread = L[0] - k, 0
            else:
                at = n0
                for x in xs[:-1]:
                    nxt = node()
                    wire(x, at, nxt)
                    at = nxt
                wire(xs[-1], at, n1); gap, spread = sum(L) - k, len(xs)
                line0 = line0 or n0
            wire(f, n1, None)
            chains.append([e, f]); exact.append([gap])
            kinds[kind].append((len(chains) - 1, 0, spread))
            if kind == "member":
                chains.append([xs[0]]); exact.append([])
    for x in short(4) or []:
        wire(x, None, hub or line0)
    # what is left: pairs that meet in a node (adjacent) and pairs that do not (a fixed gap; the restatement says what they are)
    edited = apply(edges, edits)
    rest = longs + shorts
    while len(rest) >= 2:
        e = rest.pop(0)
        near = [f for f in rest if edited[f][0] == edited[e][1]]
        f = near[0] if near else rest[0]
        rest.remove(f)
        chains.append([e, f]); exact.append([25])
    return edits, chains, exact, kinds


def gaps(exact, d):
    return [[L + d for L in g] for g in exact]
