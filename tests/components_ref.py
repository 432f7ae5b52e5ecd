"""GraphBuilder.scala:37-54 restated on strings: the components of a graph, what the builder reports of them, and the one it
keeps.  The device (gk_graph_component_stats, gk_graph_retain_largest) is held to this per component in
tests/test_small_grid_gpu.py, and this file to hand-written graphs and to the oracle in tests/test_components_cpu.py.

Input: a canonical (nodes, edges) pair as HipGraph.canonical() gives it — `nodes` a list of k-mer strings, `edges` a list of
(start k-mer, end k-mer, seq).  A node is identified by its k-mer: graphs with node copies (after a node split) are outside this
restatement.  Every start and end of an edge must be among the nodes.

  * components          :37  graph.components: the weakly connected components (an edge joins its start and its end)
  * node count          :40  components.groupBy(_.size)
  * length              :44  comp.flatMap(_.outEdges.values).map(_.seq.size).sum: the edges that START in the component, by the
                             length of their sequences (an edge starts and ends in the same component by construction)
  * the retained one    :52  components.maxBy(_.size); among several of that size the one holding the smallest k-mer

"Smallest" is the order of oracle/gk_oracle.c (gko_kmer_cmp) and of the node ids it hands out: a k-mer is the unsigned integer
pair (hi, lo) with base i in bits 2i of lo (i < 32) or bits 2(i - 32) of hi, A = 0, G = 1, C = 2, T = 3; hi decides, then lo.
In words: the LAST base weighs most, and A < G < C < T.
"""
CODE = {"A": 0, "G": 1, "C": 2, "T": 3}


def kmer_key(s):
    """the (hi, lo) pair of oracle/gk_oracle.c for a k-mer of at most 64 bases"""
    lo = hi = 0
    for i, c in enumerate(s):
        if i < 32:
            lo |= CODE[c] << (2 * i)
        else:
            hi |= CODE[c] << (2 * (i - 32))
    return hi, lo


def components(nodes, edges):
    """-> a list of components, each (sorted list of its nodes by kmer_key, node count, summed length of the edges starting in it)"""
    parent = {s: s for s in nodes}
    assert len(parent) == len(nodes), "a node twice: node copies are outside this restatement"

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b, _q in edges:
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[ra] = rb
    members, length = {}, {}
    for s in nodes:
        members.setdefault(find(s), []).append(s)
    for a, _b, q in edges:
        r = find(a)
        length[r] = length.get(r, 0) + len(q)
    return [(sorted(ms, key=kmer_key), len(ms), length.get(r, 0)) for r, ms in members.items()]


def stats(nodes, edges):
    """-> the sorted list of (node count, length) pairs, one per component"""
    return sorted((n, ln) for _ms, n, ln in components(nodes, edges))


def histograms(nodes, edges):
    """-> (hist, hist2) of GraphBuilder.scala:40-47: sorted lists of (node count, components) and (length, components)"""
    h1, h2 = {}, {}
    for n, ln in stats(nodes, edges):
        h1[n] = h1.get(n, 0) + 1
        h2[ln] = h2.get(ln, 0) + 1
    return sorted(h1.items()), sorted(h2.items())


def retained(nodes, edges):
    """-> (nodes, edges) of the component that is kept, both in the order given; ([], []) of the empty graph"""
    comps = components(nodes, edges)
    if not comps:
        return [], []
    best = max(n for _ms, n, _ln in comps)
    keep = set(min((ms for ms, n, _ln in comps if n == best), key=lambda ms: kmer_key(ms[0])))
    return [s for s in nodes if s in keep], [e for e in edges if e[0] in keep and e[1] in keep]


def tied_for_largest(nodes, edges):
    """-> the components of maximal node count, each as its sorted node list (the tie the retain rule has to break)"""
    comps = components(nodes, edges)
    best = max((n for _ms, n, _ln in comps), default=0)
    return [ms for ms, n, _ln in comps if n == best]
