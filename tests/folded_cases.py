"""What the folded-graph tests share: a genome that holds the structures on which the strand-symmetry arguments of
include/genome_amd.h have to work, the reads cut from it, and the oracle's graph of those reads in the forms the restatements take.
No device code: seeds are chosen on the CPU (the convention of insert_cases.py), tests/test_folded_cpu.py asserts on the oracle and
the restatements alone that every structure is there, and tests/test_folded_gpu.py holds the kernels to the same restatements.

The structures, each between random spacers (`drop` leaves one out: the census must then fail):
  tandem     a unit U of k + 2 .. 3k bases twice in a row: a cycle through two nodes, so that the paths from the edge before it to
             the edge after it run 0, 1, 2, .. times round the unit; and a unit V three times in a row and closed on its first k
             bases, V V V V[:k]: entry and exit are one node, the cycle is one edge whose start node is its end node;
  inverted   W, a short inner spacer, rc(W), |W| > k: an edge and its twin on one strand, and between them two parallel edges that
             run from a node to its reverse complement;
  hairpin    X rc(X), |X| >= k: a self-twin edge; at even k its centre window is a palindrome;
  homopolymer  a run of k + 5 equal bases, a self-loop of one base whose twin is another self-loop, and (AC) * k, a two-cycle;
  palnode    even k only: the k-long palindrome Y rc(Y) between two different pairs of flanks, a node that is its own reverse
             complement.
"""
import random

from genome_amd import dna
from contigs_ref import classify
from fillgaps_ref import fill
from insert_ref import CLASSES as INSERT_CLASSES
from insert_ref import index_graph, pair_distances
from judge_ref import PLACE_CLASSES, place
from links_cases import oracle_graph
from links_ref import CLASSES as LINK_CLASSES
from links_ref import JOIN_STATS, joins, pair_links
from oracle import oracle as O
from oracle import pyref as R
from pairs_ref import oracle_canonical
from spans_ref import SPLIT_STATS
from spans_ref import STATS as SPAN_STATS
from spans_ref import split_edges, thread_spans
from thread_cases import cut_reads, lengths_for, tiling
from thread_ref import STATS as THREAD_STATS
from thread_ref import thread_reads, twin_edges

KS = (11, 12, 34, 64)
STRUCTURES = ("tandem", "inverted", "hairpin", "homopolymer", "palnode")
MAX_GENOME = 1500
TILE, STEP = 120, 7
INS = (45, 80)
BINS = 96                     # gk_graph_pair_distances' bins: max_dist = 95, a little above the largest insert
# variant -> (substitution rate, count filter)
VARIANTS = {"clean": (0.0, 1), "noisy": (0.01, 2)}
# the smallest seed at which the clean variant fills every class tests/test_folded_cpu.py asks for (chosen on the CPU)
SEEDS = {11: 1, 12: 1, 34: 4, 64: 1}


def rand_seq(rnd, n):
    return "".join(rnd.choice("AGCT") for _ in range(n))


def parts(seed, k, drop=None):
    """the named pieces of the genome in order, spacers included -> [(name, sequence)]"""
    rnd = random.Random(seed * 1000 + k)
    hi = 120 if k < 30 else 60 if k < 50 else 34                     # the spacers' upper bound keeps the genome within MAX_GENOME
    out = []

    def spacer():
        out.append(("spacer", rand_seq(rnd, rnd.randint(30, hi))))

    def unit():
        return rand_seq(rnd, rnd.randint(k + 2, 3 * k if k < 50 else k + 12))               # (k = 64: 1500 bases hold no more)

    spacer()
    # every structure draws its random numbers whether it is kept or not, so that dropping one leaves the others as they were
    U, V = unit(), unit()
    # W's edge has |W| - k bases.  Small k: long enough that a pair of INS lies on it whole, so that its copies fill `ambiguous`;
    # large k: short enough that a fragment of at most INS[1] bases reaches from it into its twin
    W, inner = rand_seq(rnd, k + (rnd.randint(40, 48) if k < 30 else rnd.randint(10, 14))), rand_seq(rnd, 3)
    X = rand_seq(rnd, k + rnd.randint(0, 6))
    base = rnd.choice("AGCT")
    Y = rand_seq(rnd, k // 2)
    mid = rand_seq(rnd, rnd.randint(30, hi))
    if drop != "tandem":
        out.append(("tandem2", U * 2)); spacer()
        out.append(("tandem3", V * 3 + V[:k])); spacer()
    if drop != "inverted":
        out.append(("inverted", W + inner + R.rev_comp(W))); spacer()
    if drop != "hairpin":
        out.append(("hairpin", X + R.rev_comp(X))); spacer()
    if drop != "homopolymer":
        out.append(("homopolymer", base * (k + 5))); spacer()
        out.append(("two_cycle", "AC" * k)); spacer()
    if k % 2 == 0 and drop != "palnode":
        out.append(("palnode", Y + R.rev_comp(Y))); out.append(("spacer", mid))
        out.append(("palnode", Y + R.rev_comp(Y))); spacer()
    return out


def folded_genome(seed, k, drop=None):
    g = "".join(s for _, s in parts(seed, k, drop))
    assert len(g) <= MAX_GENOME
    return g


def where(seed, k, name):
    """(offset, length) of the first piece called `name` in folded_genome(seed, k)"""
    at = 0
    for n, s in parts(seed, k):
        if n == name:
            return at, len(s)
        at += len(s)
    raise KeyError(name)


def cut_pairs(seed, g, k, npairs, err=0.0):
    """mates of k + 9 bases (shorter where the fragment is), inserts INS, from both strands: [mate 1, mate 2, mate 1, ..]"""
    rnd = random.Random(seed * 104729 + 3)
    L = k + 9
    noisy = lambda m: "".join(c if rnd.random() >= err else rnd.choice([x for x in "AGCT" if x != c]) for c in m)
    reads = []
    for _ in range(npairs):
        n = rnd.randint(*INS)
        s = rnd.randrange(0, len(g) - n)
        frag = g[s:s + n]
        if rnd.random() < 0.5:
            frag = R.rev_comp(frag)
        m1, m2 = frag[:L], R.rev_comp(frag)[:L]
        reads += [noisy(m1), noisy(m2)] if err else [m1, m2]
    return reads


class Case:
    """one (k, seed, variant): genome, the reads the graph is built from, singles, pairs, count filter"""

    def __init__(self, k, seed, variant, drop=None, nsingles=400, npairs=800):
        err, self.min_count = VARIANTS[variant]
        self.k, self.seed, self.variant = k, seed, variant
        self.genome = folded_genome(seed, k, drop)
        self.singles = cut_reads(seed, self.genome, lengths_for(k, nsingles, seed), err)
        self.singles += [self.genome[i:i + 150] for i in range(0, len(self.genome) - 150, 11)]
        assert len(self.singles) <= 600
        self.pairs = cut_pairs(seed, self.genome, k, npairs, err)
        self.npairs = npairs
        self.graph_reads = tiling(self.genome, TILE, STEP)
        if err:                                  # the noisy reads are in the table; the filter keeps what was seen twice
            self.graph_reads = self.graph_reads + self.singles + self.pairs

    def canonical(self):
        """the oracle's (sorted node k-mers, sorted (start, end, seq))"""
        ref = O.PMap(self.k, 1)
        ref.count_reads(dna.reads_to_bin(self.graph_reads), len(self.graph_reads))
        if self.min_count > 1:
            ref.delete_lt(self.min_count)
        return oracle_canonical(O.Graph(ref))

    def counts(self):
        """the count table as tips_ref takes it: stored k-mer -> count"""
        ref = O.PMap(self.k, 1)
        ref.count_reads(dna.reads_to_bin(self.graph_reads), len(self.graph_reads))
        if self.min_count > 1:
            ref.delete_lt(self.min_count)
        lo, hi, cnt = ref.export_sorted()
        return {dna.unpack(int(a), int(b), self.k): int(c) for a, b, c in zip(lo, hi, cnt)}

    def indexed(self):
        """links_cases.oracle_graph: (index, edge lengths, content keys, paths)"""
        return oracle_graph(self.k, self.graph_reads, self.min_count)

    def by_index(self):
        """the graph as thread_ref and spans_ref take it: (node k-mers, edges (start index, end index, seq), content keys)"""
        nodes, oedges = self.canonical()
        at = {s: i for i, s in enumerate(nodes)}
        assert len(at) == len(nodes)
        return nodes, [(at[s], at[t], q) for s, t, q in oedges], [(s, dna.BASES.index(q[0])) for s, _, q in oedges]


_cache = {}


def case(k, seed, variant):
    key = (k, seed, variant)
    if key not in _cache:
        _cache[key] = Case(k, seed, variant)
    return _cache[key]


# ---- the census: what the oracle and the restatements find in a case, on the CPU ----------------------------------------------

LINK_SPAN = 100                       # gk_graph_pair_links' max_span = LINK_SPAN + k, min_len = 0 (the folded edges are short)
SUPPORT = 3


def split_graph(c, cutoff=1):
    """the oracle's graph after spans_ref.split_edges at `cutoff` with the spans of the singles -> (nodes, edges, stats); the copies
    it leaves share every k-mer of the spanned edge, which is what fills the position-list classes"""
    nodes, edges, _ = c.by_index()
    spans, _ = thread_spans(c.k, nodes, edges, c.singles)
    return split_edges(nodes, edges, spans, cutoff)


def place_on(k, nodes, edges, records):
    return place(k, dict(enumerate(nodes)), {e: (nodes[s], q) for e, (s, _, q) in enumerate(edges)}, records)


def census(c):
    """every figure tests/test_folded_cpu.py asserts on -> dict"""
    k = c.k
    nodes, edges, _ = c.by_index()
    paths = [nodes[s] + q for s, _, q in edges]
    out = dict(genome=len(c.genome), nodes=len(nodes), edges=len(edges))
    out["start_is_end"] = sum(s == t for s, t, _ in edges)
    by_path = {p: e for e, p in enumerate(paths)}
    # the homopolymer: a self-loop of one base whose twin is another self-loop
    out["one_base_loops"] = sum(s == t and len(q) == 1 and by_path[R.rev_comp(nodes[s] + q)] != e and edges[by_path[R.rev_comp(nodes[s] + q)]][0] ==
                                edges[by_path[R.rev_comp(nodes[s] + q)]][1] for e, (s, t, q) in enumerate(edges))
    out["self_twin"] = sum(classify(p) == "self_twin" for p in paths)
    out["end_is_rc_start"] = sum(nodes[t] == R.rev_comp(nodes[s]) for s, t, _ in edges)
    out["palindromic_nodes"] = sum(n == R.rev_comp(n) for n in nodes)
    index, lens = index_graph(k, [(nodes[s], q) for s, _, q in edges], nodes=nodes)
    out["palindromic_windows"] = sum(w == R.rev_comp(w) for w, v in index.items() if v[0][0] == "E")
    out["two_positions"] = sum(len(v) >= 2 for v in index.values())
    twin = twin_edges(k, nodes, edges)
    sup, st = thread_reads(k, nodes, edges, c.singles)
    out["thread"] = tuple(st[x] for x in THREAD_STATS)
    out["crossings_e_is_f"] = sum(n for (e, f), n in sup.items() if e == f)
    spans, st = thread_spans(k, nodes, edges, c.singles)
    out["spans"] = tuple(st[x] for x in SPAN_STATS)
    out["spans_through_a_loop"] = sum(e == m or m == f for e, m, f in spans)
    for cutoff in (1, 3):
        out["split%d" % cutoff] = tuple(split_edges(nodes, edges, spans, cutoff)[2][x] for x in SPLIT_STATS)
    _, cls = pair_distances(k, index, lens, c.pairs, c.npairs, BINS)
    out["insert"] = tuple(cls[x] for x in INSERT_CLASSES)
    links, cls = pair_links(k, index, lens, c.pairs, c.npairs, 0, LINK_SPAN + k)
    out["links"] = tuple(cls[x] for x in LINK_CLASSES)
    out["links_e_twin_e"] = sum(f == twin[e] for e, f in links)
    out["links_e_e"] = sum(e == f for e, f in links)
    out["joins"] = tuple(joins(links, SUPPORT)[1][x] for x in JOIN_STATS)
    pst, _ = place_on(k, nodes, edges, [c.genome])
    out["place"] = tuple(pst[x] for x in PLACE_CLASSES)
    # after the split at cutoff 1: the copies share k-mers
    n2, e2, _ = split_graph(c)
    i2, l2 = index_graph(k, [(n2[s], q) for s, _, q in e2], nodes=n2)
    out["split_two_positions"] = sum(len(v) >= 2 for v in i2.values())
    out["split_thread"] = tuple(thread_reads(k, n2, e2, c.singles)[1][x] for x in THREAD_STATS)
    out["split_spans"] = tuple(thread_spans(k, n2, e2, c.singles)[1][x] for x in SPAN_STATS)
    out["split_insert"] = tuple(pair_distances(k, i2, l2, c.pairs, c.npairs, BINS)[1][x] for x in INSERT_CLASSES)
    out["split_links"] = tuple(pair_links(k, i2, l2, c.pairs, c.npairs, 0, LINK_SPAN + k)[1][x] for x in LINK_CLASSES)
    pst, _ = place_on(k, n2, e2, [c.genome])
    out["split_place"] = tuple(pst[x] for x in ("fwd_repetitive", "rev_repetitive") + PLACE_CLASSES)
    sn, se = simplify(n2, e2)
    out["split_simplified"] = (sum(x is not None for x in sn), sum(x is not None for x in se))
    if c.variant == "clean":
        by_len = {e: (s, t, len(q)) for e, (s, t, q) in enumerate(edges)}
        out["fill"] = tuple(tuple(fill(by_len, k, ch, gp, tol, me, mp)[2]["classes"][0]) for ch, gp, tol, me, mp in fill_cases(by_len, k, tandem_unit(c)))
    return out


# ---- MapGraph.simplifyGraph (Graph.scala:211-230), restated by id ---------------------------------------------------------------

def simplify(nodes, edges):
    """nodes: k-mers by id (None = dead); edges: by id, (start id, end id, sequence) or None -> the same after simplifyGraph: in id
    order, a node without edges goes; a node with one way in and one way out goes, and its two edges become one appended edge
    (a loop that is both goes with it).  The content that is left does not depend on the order."""
    nodes, edges = list(nodes), list(edges)
    ins, outs = {}, {}
    for e, x in enumerate(edges):
        if x is not None:
            outs.setdefault(x[0], []).append(e)
            ins.setdefault(x[1], []).append(e)

    def remove(e):
        outs[edges[e][0]].remove(e)
        ins[edges[e][1]].remove(e)
        edges[e] = None

    for n in range(len(nodes)):
        if nodes[n] is None:
            continue
        i, o = ins.get(n, []), outs.get(n, [])
        if not i and not o:
            nodes[n] = None
        elif len(i) == 1 and len(o) == 1:
            e1, e2 = i[0], o[0]
            if e1 == e2:
                remove(e1)
            else:
                (s, _, q1), (_, t, q2) = edges[e1], edges[e2]
                remove(e1); remove(e2)
                edges.append((s, t, q1 + q2))
                outs.setdefault(s, []).append(len(edges) - 1)
                ins.setdefault(t, []).append(len(edges) - 1)
            nodes[n] = None
    return nodes, edges


def content(nodes, edges):
    """by-id lists -> what pairs_ref.gpu_canonical gives: (sorted node k-mers, sorted (start k-mer, end k-mer, sequence))"""
    return sorted(x for x in nodes if x is not None), sorted((nodes[x[0]], nodes[x[1]], x[2]) for x in edges if x is not None)


# ---- gap filling through the tandem cycle ----------------------------------------------------------------------------------------

def tandem_unit(c):
    return where(c.seed, c.k, "tandem2")[1] // 2


def cycle_gadgets(by_len, unit):
    """by_len: {edge id: (start node, end node, len)}.  The two-node cycle of the unit U U, on either strand: a = n1 -> n2 and b =
    n2 -> n1 with len_a + len_b = |U|, n1 entered by b and one edge e more and left by a alone, n2 left by b and one edge f more
    and entered by a alone -> [(e, f, a, b)] in ascending e"""
    ins, outs = {}, {}
    for x, (s, t, _n) in by_len.items():
        outs.setdefault(s, []).append(x)
        ins.setdefault(t, []).append(x)
    found = []
    for a, (n1, n2, la) in by_len.items():
        if n1 == n2 or outs[n1] != [a] or ins[n2] != [a] or len(ins.get(n1, [])) != 2 or len(outs.get(n2, [])) != 2:
            continue
        for b in outs[n2]:
            if by_len[b][1] == n1 and la + by_len[b][2] == unit and b in ins[n1]:
                (e,), (f,) = [x for x in ins[n1] if x != b], [x for x in outs[n2] if x != b]
                if len({e, f, a, b}) == 4:
                    found.append((e, f, a, b))
    return sorted(found)


def fill_cases(by_len, k, unit):
    """the chain (e, f) of the first gadget: the paths from e to f are a, a b a, a b a b a, .. with gap lengths L_r = len_a - k +
    r |U|.  -> [(chains, gaps, tol, max_edges, max_paths)]: the gap estimate at L_0 exactly (one path within tol), at L_1 exactly
    (one path, which holds a twice), between L_0 and L_1 with a tolerance that reaches both (two), two bases off L_0 with
    tolerance 1 (none), and the second again with max_paths = 2 (a, a b, a b a forward and a, b a, e a backward: the tree overflows
    from both sides)"""
    e, f, a, _b = cycle_gadgets(by_len, unit)[0]
    L0 = by_len[a][2] - k
    half = unit // 2
    return [([[e, f]], [[L0]], 0, 16, 256), ([[e, f]], [[L0 + unit]], 0, 16, 256), ([[e, f]], [[L0 + half]], unit - half, 16, 256),
            ([[e, f]], [[L0 + 2]], 1, 16, 256), ([[e, f]], [[L0 + unit]], 0, 16, 2)]


FILL_CLASSES_WANTED = (("filled",), ("shared",), ("ambiguous",), ("none",), ("overflow",))


# census() of every case, measured on the CPU with the oracle and the restatements; never read off the device
TABLE = {(11, 'clean'): {'genome': 935,
                 'nodes': 34,
                 'edges': 49,
                 'start_is_end': 4,
                 'one_base_loops': 2,
                 'self_twin': 5,
                 'end_is_rc_start': 7,
                 'palindromic_nodes': 0,
                 'palindromic_windows': 0,
                 'two_positions': 0,
                 'thread': (449, 107362, 0, 0, 102168, 0, 5194),
                 'crossings_e_is_f': 1568,
                 'spans': (449, 5194, 4412, 0, 782),
                 'spans_through_a_loop': 12,
                 'split1': (11, 5, 0, 2, 4, 5, 10),
                 'split3': (11, 5, 0, 2, 4, 5, 10),
                 'insert': (1600, 0, 0, 1158, 0, 24, 0, 331, 87),
                 'links': (1600, 0, 0, 160, 442, 0, 0, 998),
                 'links_e_twin_e': 1,
                 'links_e_e': 0,
                 'joins': (59, 51, 2, 17, 17),
                 'place': (16, 3, 8, 11, 11),
                 'split_two_positions': 150,
                 'split_thread': (449, 107362, 0, 19120, 84228, 0, 4014),
                 'split_spans': (449, 4014, 3506, 102, 406),
                 'split_insert': (1600, 0, 0, 1158, 8, 24, 0, 323, 87),
                 'split_links': (1600, 0, 440, 130, 434, 0, 0, 596),
                 'split_place': (150, 150, 26, 0, 6, 11, 11),
                 'split_simplified': (24, 34),
                 'fill': (('filled',), ('shared',), ('ambiguous',), ('none',), ('overflow',))},
 (11, 'noisy'): {'genome': 935,
                 'nodes': 450,
                 'edges': 528,
                 'start_is_end': 4,
                 'one_base_loops': 2,
                 'self_twin': 8,
                 'end_is_rc_start': 8,
                 'palindromic_nodes': 0,
                 'palindromic_windows': 0,
                 'two_positions': 0,
                 'thread': (449, 107362, 7108, 0, 76362, 420, 23472),
                 'crossings_e_is_f': 1294,
                 'spans': (449, 23472, 22134, 564, 774),
                 'spans_through_a_loop': 22,
                 'split1': (42, 0, 0, 40, 2, 0, 0),
                 'split3': (42, 0, 0, 4, 38, 0, 0),
                 'insert': (1600, 254, 0, 1260, 0, 0, 0, 86, 0),
                 'links': (1600, 254, 0, 554, 86, 0, 0, 706),
                 'links_e_twin_e': 1,
                 'links_e_e': 0,
                 'joins': (337, 73, 9, 18, 18),
                 'place': (367, 27, 22, 56, 56),
                 'split_two_positions': 0,
                 'split_thread': (449, 107362, 7108, 0, 76362, 420, 23472),
                 'split_spans': (449, 23472, 22134, 564, 774),
                 'split_insert': (1600, 254, 0, 1260, 0, 0, 0, 86, 0),
                 'split_links': (1600, 254, 0, 554, 86, 0, 0, 706),
                 'split_place': (0, 0, 367, 27, 22, 56, 56),
                 'split_simplified': (450, 528)},
 (12, 'clean'): {'genome': 1094,
                 'nodes': 37,
                 'edges': 55,
                 'start_is_end': 6,
                 'one_base_loops': 2,
                 'self_twin': 1,
                 'end_is_rc_start': 5,
                 'palindromic_nodes': 1,
                 'palindromic_windows': 1,
                 'two_positions': 0,
                 'thread': (463, 111010, 0, 0, 106302, 0, 4708),
                 'crossings_e_is_f': 1142,
                 'spans': (463, 4708, 3926, 0, 782),
                 'spans_through_a_loop': 12,
                 'split1': (9, 5, 0, 2, 2, 5, 10),
                 'split3': (9, 5, 0, 2, 2, 5, 10),
                 'insert': (1600, 0, 0, 1040, 0, 12, 0, 443, 105),
                 'links': (1600, 0, 0, 122, 560, 0, 0, 918),
                 'links_e_twin_e': 1,
                 'links_e_e': 0,
                 'joins': (55, 49, 10, 12, 12),
                 'place': (20, 3, 6, 13, 13),
                 'split_two_positions': 127,
                 'split_thread': (463, 111010, 0, 14760, 92558, 0, 3692),
                 'split_spans': (463, 3692, 3076, 117, 499),
                 'split_insert': (1600, 0, 0, 1040, 8, 12, 0, 435, 105),
                 'split_links': (1600, 0, 316, 86, 552, 0, 0, 646),
                 'split_place': (127, 127, 30, 0, 4, 13, 13),
                 'split_simplified': (27, 40),
                 'fill': (('filled',), ('shared',), ('ambiguous',), ('none',), ('overflow',))},
 (12, 'noisy'): {'genome': 1094,
                 'nodes': 469,
                 'edges': 539,
                 'start_is_end': 2,
                 'one_base_loops': 2,
                 'self_twin': 1,
                 'end_is_rc_start': 1,
                 'palindromic_nodes': 1,
                 'palindromic_windows': 1,
                 'two_positions': 0,
                 'thread': (463, 111010, 7430, 0, 82880, 336, 20364),
                 'crossings_e_is_f': 422,
                 'spans': (463, 20364, 19008, 547, 809),
                 'spans_through_a_loop': 6,
                 'split1': (54, 2, 4, 44, 4, 2, 4),
                 'split3': (54, 2, 4, 2, 46, 2, 4),
                 'insert': (1600, 276, 0, 1292, 0, 2, 0, 30, 0),
                 'links': (1600, 276, 0, 490, 32, 0, 0, 802),
                 'links_e_twin_e': 1,
                 'links_e_e': 0,
                 'joins': (415, 74, 16, 15, 15),
                 'place': (336, 23, 20, 80, 80),
                 'split_two_positions': 18,
                 'split_thread': (463, 111010, 7430, 1180, 81970, 330, 20100),
                 'split_spans': (463, 20100, 18716, 591, 793),
                 'split_insert': (1600, 276, 0, 1292, 0, 2, 0, 30, 0),
                 'split_links': (1600, 276, 56, 468, 32, 0, 0, 768),
                 'split_place': (18, 18, 340, 23, 18, 80, 80),
                 'split_simplified': (465, 533)},
 (34, 'clean'): {'genome': 1090,
                 'nodes': 33,
                 'edges': 49,
                 'start_is_end': 4,
                 'one_base_loops': 2,
                 'self_twin': 1,
                 'end_is_rc_start': 5,
                 'palindromic_nodes': 1,
                 'palindromic_windows': 1,
                 'two_positions': 0,
                 'thread': (463, 93012, 0, 0, 86784, 0, 6228),
                 'crossings_e_is_f': 736,
                 'spans': (463, 6228, 5426, 0, 802),
                 'spans_through_a_loop': 12,
                 'split1': (9, 5, 0, 2, 2, 5, 10),
                 'split3': (9, 5, 0, 2, 2, 5, 10),
                 'insert': (1600, 0, 0, 738, 0, 84, 0, 645, 133),
                 'links': (1600, 0, 0, 194, 862, 0, 0, 544),
                 'links_e_twin_e': 1,
                 'links_e_e': 0,
                 'joins': (39, 34, 10, 9, 9),
                 'place': (20, 3, 4, 11, 11),
                 'split_two_positions': 181,
                 'split_thread': (463, 93012, 0, 16750, 70954, 0, 5308),
                 'split_spans': (463, 5308, 4804, 63, 441),
                 'split_insert': (1600, 0, 0, 738, 104, 80, 0, 545, 133),
                 'split_links': (1600, 0, 468, 164, 758, 0, 0, 210),
                 'split_place': (181, 181, 30, 0, 2, 11, 11),
                 'split_simplified': (23, 34),
                 'fill': (('filled',), ('shared',), ('ambiguous',), ('none',), ('overflow',))},
 (34, 'noisy'): {'genome': 1090,
                 'nodes': 521,
                 'edges': 461,
                 'start_is_end': 2,
                 'one_base_loops': 2,
                 'self_twin': 1,
                 'end_is_rc_start': 1,
                 'palindromic_nodes': 1,
                 'palindromic_windows': 1,
                 'two_positions': 0,
                 'thread': (463, 93012, 16728, 0, 63886, 438, 11960),
                 'crossings_e_is_f': 342,
                 'spans': (463, 11960, 10926, 361, 673),
                 'spans_through_a_loop': 8,
                 'split1': (30, 0, 6, 22, 2, 0, 0),
                 'split3': (30, 0, 6, 2, 22, 0, 0),
                 'insert': (1600, 714, 0, 780, 0, 0, 0, 97, 9),
                 'links': (1600, 714, 0, 262, 106, 0, 0, 518),
                 'links_e_twin_e': 1,
                 'links_e_e': 0,
                 'joins': (257, 46, 24, 6, 6),
                 'place': (342, 13, 32, 37, 37),
                 'split_two_positions': 0,
                 'split_thread': (463, 93012, 16728, 0, 63886, 438, 11960),
                 'split_spans': (463, 11960, 10926, 361, 673),
                 'split_insert': (1600, 714, 0, 780, 0, 0, 0, 97, 9),
                 'split_links': (1600, 714, 0, 262, 106, 0, 0, 518),
                 'split_place': (0, 0, 342, 13, 32, 37, 37),
                 'split_simplified': (521, 461)},
 (64, 'clean'): {'genome': 1305,
                 'nodes': 27,
                 'edges': 41,
                 'start_is_end': 6,
                 'one_base_loops': 2,
                 'self_twin': 1,
                 'end_is_rc_start': 5,
                 'palindromic_nodes': 1,
                 'palindromic_windows': 1,
                 'two_positions': 0,
                 'thread': (482, 86148, 0, 0, 81598, 0, 4550),
                 'crossings_e_is_f': 3156,
                 'spans': (482, 4550, 3782, 0, 768),
                 'spans_through_a_loop': 18,
                 'split1': (5, 5, 0, 0, 0, 5, 10),
                 'split3': (5, 5, 0, 0, 0, 5, 10),
                 'insert': (744, 0, 0, 130, 0, 2, 0, 229, 383),
                 'links': (744, 0, 0, 64, 614, 0, 0, 66),
                 'links_e_twin_e': 0,
                 'links_e_e': 0,
                 'joins': (26, 12, 8, 1, 1),
                 'place': (10, 3, 6, 11, 11),
                 'split_two_positions': 107,
                 'split_thread': (482, 86148, 0, 6996, 75232, 0, 3920),
                 'split_spans': (482, 3920, 3440, 21, 459),
                 'split_insert': (744, 0, 0, 130, 34, 2, 0, 210, 368),
                 'split_links': (744, 0, 96, 52, 580, 0, 0, 16),
                 'split_place': (107, 107, 20, 0, 4, 11, 11),
                 'split_simplified': (17, 26),
                 'fill': (('filled',), ('shared',), ('ambiguous',), ('none',), ('overflow',))},
 (64, 'noisy'): {'genome': 1305,
                 'nodes': 267,
                 'edges': 223,
                 'start_is_end': 2,
                 'one_base_loops': 2,
                 'self_twin': 1,
                 'end_is_rc_start': 3,
                 'palindromic_nodes': 1,
                 'palindromic_windows': 1,
                 'two_positions': 0,
                 'thread': (482, 86148, 28438, 0, 52540, 252, 4918),
                 'crossings_e_is_f': 168,
                 'spans': (482, 4918, 4224, 159, 535),
                 'spans_through_a_loop': 6,
                 'split1': (14, 2, 0, 8, 4, 2, 4),
                 'split3': (14, 2, 0, 4, 8, 2, 4),
                 'insert': (740, 506, 0, 86, 0, 0, 0, 87, 61),
                 'links': (740, 506, 0, 56, 148, 0, 0, 30),
                 'links_e_twin_e': 0,
                 'links_e_e': 0,
                 'joins': (20, 2, 2, 0, 0),
                 'place': (172, 5, 10, 18, 18),
                 'split_two_positions': 24,
                 'split_thread': (482, 86148, 28438, 1146, 51586, 250, 4728),
                 'split_spans': (482, 4728, 4070, 179, 479),
                 'split_insert': (740, 506, 0, 86, 2, 0, 0, 85, 61),
                 'split_links': (740, 506, 6, 54, 146, 0, 0, 28),
                 'split_place': (24, 24, 176, 3, 10, 18, 18),
                 'split_simplified': (263, 217)}}
