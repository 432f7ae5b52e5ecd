"""A string-based restatement of the insert-range rules of include/genome_amd.h ("the insert range"), for the tests.  It never
touches the device's position map: a graph is given as (start k-mer, sequence) strings, every k-window of every edge is indexed
by its text, and pair orientations are classified by the rule's table, one `if` per row.  Plus gk_insert_range in Python
integers."""
from oracle import pyref as R

CLASSES = ("orientations", "unplaced", "repetitive", "apart", "ambiguous", "reversed", "beyond", "near_end", "counted")
MAX_LIST = 16


def index_graph(k, edges, nodes=None):
    """edges: [(start k-mer, sequence)]; edge e is its index in the list.  The window at distance d of start ++ sequence is an
    EDGE position (e, d) for d = 1 .. len - 1 (Graph.getGraphMap, Graph.scala:90-119); distance 0 and distance len are the
    start and end NODE.  nodes: the node k-mers, one entry per node (copies of a split node repeat); None: the distinct start
    and end k-mers of the edges.  -> ({k-mer: [("N", i) | ("E", e, d)]}, [len of edge e])"""
    index, lens = {}, []
    if nodes is None:
        nodes = sorted({s for s, _ in edges} | {(s + q)[-k:] for s, q in edges})
    for i, s in enumerate(nodes):
        assert len(s) == k
        index.setdefault(s, []).append(("N", i))
    for e, (s, q) in enumerate(edges):
        assert len(s) == k and len(q) >= 1
        path = s + q
        lens.append(len(q))
        for d in range(1, len(q)):
            index.setdefault(path[d:d + k], []).append(("E", e, d))
    return index, lens


def classify(P1, P2, k, lens, max_dist):
    """one orientation -> (class name, D or None)"""
    if not P1 or not P2:
        return "unplaced", None
    if len(P1) > MAX_LIST or len(P2) > MAX_LIST:
        return "repetitive", None
    C = [(a, b) for a in P1 for b in P2 if a[0] == "E" and b[0] == "E" and a[1] == b[1]]
    if not C:
        return "apart", None
    if len(C) >= 2:
        return "ambiguous", None
    (a, b), = C
    D = b[2] - a[2] + k
    if D < k:
        return "reversed", D
    if D > max_dist:
        return "beyond", D
    if a[2] + max_dist - k >= lens[a[1]]:
        return "near_end", D
    return "counted", D


def pair_distances(k, index, lens, reads, npairs, bins):
    """the first `npairs` pairs of reads = [mate 1, mate 2, mate 1, ...] -> (hist as a list of bins ints, {class: count})"""
    hist, cls = [0] * bins, dict.fromkeys(CLASSES, 0)
    for p in range(min(npairs, len(reads) // 2)):
        m1, m2 = reads[2 * p], reads[2 * p + 1]
        if len(m1) < k or len(m2) < k:
            continue
        for x, y in ((m1, m2), (m2, m1)):
            c, D = classify(index.get(x[:k], []), index.get(R.rev_comp(y[:k]), []), k, lens, bins - 1)
            cls["orientations"] += 1
            cls[c] += 1
            if c == "counted":
                hist[D] += 1
    return hist, cls


def insert_range(hist, trim, min_observations):
    """gk_insert_range -> (lo, hi, median); (0, 0, 0) = no estimate"""
    n = sum(int(x) for x in hist)
    if n < max(min_observations, 1):
        return 0, 0, 0
    cum, lo, hi, med = 0, None, None, None
    for D, c in enumerate(hist):
        cum += int(c)
        if lo is None and 1000 * cum > trim * n:
            lo = D
        if med is None and 2 * cum >= n:
            med = D
        if hi is None and 1000 * cum >= (1000 - trim) * n:
            hi = D
    return lo, hi, med
