"""The folded inputs contain what they claim (no device; the GPU file is tests/test_folded_gpu.py).  For every (k, seed) that file
uses, the oracle's graph and the restatements alone show the structures of folded_cases.py and the classes they are there to
fill; the figures are pinned in folded_cases.TABLE.  Then the hand cases that hold the restatements themselves to answers worked
out in their docstrings, on the same structures.

What cannot be, and is asserted as such:
  * a fresh graph holds no k-mer at two positions, palindromes included: a k-mer lies on one unitig, so a palindromic window lies
    on an edge that is its own twin, at its centre, once.  `repeated`, `ambiguous` and `repetitive` are therefore filled on the
    folded graph AFTER the span split at cutoff 1, whose copies share the k-mers of the spanned edge;
  * a link (e, e) is `same_edge` by the rule, a self-twin e included: the census asserts there is none;
  * with inserts of at most 80 a link (e, twin e) across the inverted repeat needs 2k + 5 <= 80: k = 64 has no such link;
  * error-free reads leave no crossing `interrupted` on a fresh graph: that class is asserted on the noisy variant and after the
    split."""
import pytest

import folded_cases as F
import tips_ref as T
from contigs_ref import classify
from insert_ref import index_graph, pair_distances
from links_ref import pair_links
from genome_amd import dna
from oracle import oracle as O
from oracle import pyref as R
from pairs_ref import oracle_canonical
from spans_ref import thread_spans

CASES = [(k, F.SEEDS[k]) for k in F.KS]


@pytest.fixture(scope="module")
def figures():
    return {(k, v): F.census(F.case(k, F.SEEDS[k], v)) for k in F.KS for v in F.VARIANTS}


@pytest.mark.parametrize("k, seed", CASES)
def test_the_genome_is_short_and_holds_every_piece(k, seed):
    names = [n for n, _ in F.parts(seed, k)]
    want = {"tandem2", "tandem3", "inverted", "hairpin", "homopolymer", "two_cycle"} | ({"palnode"} if k % 2 == 0 else set())
    assert set(names) - {"spacer"} == want and len(F.folded_genome(seed, k)) <= F.MAX_GENOME
    c = F.case(k, seed, "clean")
    assert len(c.singles) <= 600 and c.npairs <= 800 and max(len(m) for m in c.pairs) == k + 9


@pytest.mark.parametrize("k, seed", CASES)
def test_census_of_the_clean_variant(figures, k, seed):
    o = figures[(k, "clean")]
    thread, spans, ins, links, place = (dict(zip(n, o[x])) for n, x in ((F.THREAD_STATS, "thread"), (F.SPAN_STATS, "spans"), (F.INSERT_CLASSES, "insert"),
                                                                         (F.LINK_CLASSES, "links"), (F.PLACE_CLASSES, "place")))
    assert o["start_is_end"] > 0 and o["self_twin"] > 0 and o["end_is_rc_start"] > 0
    assert o["one_base_loops"] >= 2                                            # the homopolymer's loop and its twin, another loop
    if k % 2 == 0:
        assert o["palindromic_nodes"] > 0 and o["palindromic_windows"] > 0
    assert o["two_positions"] == 0                                             # (see the module's docstring)
    assert thread["repeated"] == 0 and thread["crossings"] > 0 and o["crossings_e_is_f"] > 0
    assert spans["spans"] > 0 and spans["open"] > 0 and spans["interrupted"] == 0 and o["spans_through_a_loop"] > 0
    assert dict(zip(F.SPLIT_STATS, o["split1"]))["candidates"] > 0
    assert ins["reversed"] > 0 and ins["counted"] > 0 and ins["ambiguous"] == 0
    assert links["linked"] > 0 and links["same_edge"] > 0 and o["links_e_e"] == 0
    assert (o["links_e_twin_e"] > 0) == (k != 64)
    assert dict(zip(F.JOIN_STATS, o["joins"]))["forks"] > 0
    assert place["both_strands"] > 0 and place["scattered"] > 0 and place["forward"] > 0
    # after the split the copies share k-mers: the position-list classes
    assert o["split_two_positions"] > 0
    assert dict(zip(F.THREAD_STATS, o["split_thread"]))["repeated"] > 0
    assert dict(zip(F.SPAN_STATS, o["split_spans"]))["interrupted"] > 0
    assert dict(zip(F.INSERT_CLASSES, o["split_insert"]))["ambiguous"] > 0
    # the paths round the tandem unit: one within tol, one that holds an edge twice, two, none, and a tree that overflows
    assert o["fill"] == F.FILL_CLASSES_WANTED
    assert dict(zip(F.LINK_CLASSES, o["split_links"]))["repetitive"] > 0
    assert o["split_place"][0] > 0 and o["split_place"][1] > 0                  # fwd_repetitive, rev_repetitive


@pytest.mark.parametrize("k, seed", CASES)
def test_census_of_the_noisy_variant(figures, k, seed):
    o = figures[(k, "noisy")]
    thread, spans, ins = dict(zip(F.THREAD_STATS, o["thread"])), dict(zip(F.SPAN_STATS, o["spans"])), dict(zip(F.INSERT_CLASSES, o["insert"]))
    assert thread["off_graph"] > 0 and thread["broken"] > 0 and thread["crossings"] > 0
    assert spans["spans"] > 0 and spans["interrupted"] > 0 and spans["open"] > 0
    assert ins["unplaced"] > 0 and o["self_twin"] > 0 and o["start_is_end"] > 0


@pytest.mark.parametrize("k, seed", CASES)
def test_the_candidates_of_the_split_hold_a_loop_or_a_self_twin_edge(k, seed):
    """among the candidates of spans_ref.split_edges (one way out of the start, one way into the end, two ways or more into the
    start and out of the end) there is a self-loop, a self-twin edge, or an edge that runs from a node to its reverse complement"""
    nodes, edges, _ = F.case(k, seed, "clean").by_index()
    ins, outs = {}, {}
    for e, (s, t, _q) in enumerate(edges):
        outs.setdefault(s, []).append(e)
        ins.setdefault(t, []).append(e)
    cand = [(s, t, q) for s, t, q in edges if len(outs[s]) == 1 and len(ins[t]) == 1 and len(ins.get(s, [])) >= 2 and len(outs.get(t, [])) >= 2]
    assert len(cand) == F.TABLE[(k, "clean")]["split1"][0]
    assert any(s == t or classify(nodes[s] + q) == "self_twin" or nodes[t] == R.rev_comp(nodes[s]) for s, t, q in cand)


@pytest.mark.parametrize("variant", list(F.VARIANTS))
@pytest.mark.parametrize("k, seed", CASES)
def test_the_pinned_table(figures, k, seed, variant):
    assert figures[(k, variant)] == F.TABLE[(k, variant)]


@pytest.mark.parametrize("k, seed", CASES)
def test_a_read_crosses_one_node_twice(k, seed):
    """the one read that holds the three copies of the tandem unit V crosses a node of that cycle by one (in, out) pair twice or more
    (where the flank happens to go on as V does, entry and exit lie a base apart and the cycle has two nodes: k = 12)"""
    c = F.case(k, seed, "clean")
    at, n = F.where(seed, k, "tandem3")
    nodes, edges, _ = c.by_index()
    sup, _ = F.thread_reads(k, nodes, edges, [c.genome[at - 2:at + n + 2]])
    twin = F.twin_edges(k, nodes, edges)
    assert any(cnt >= 2 and (twin[f], twin[e]) != (e, f) for (e, f), cnt in sup.items())          # (twin keys differ: one strand gave both)


@pytest.mark.parametrize("variant", list(F.VARIANTS))
@pytest.mark.parametrize("k, seed", CASES)
def test_the_simplify_restatement_is_the_oracles(k, seed, variant):
    """folded_cases.simplify on the unedited graph gives what the oracle's simplifyGraph leaves, by content"""
    c = F.case(k, seed, variant)
    ref = O.PMap(k, 1)
    ref.count_reads(dna.reads_to_bin(c.graph_reads), len(c.graph_reads))
    if c.min_count > 1:
        ref.delete_lt(c.min_count)
    og = O.Graph(ref)
    og.simplify()
    nodes, edges, _ = c.by_index()
    assert F.content(*F.simplify(nodes, edges)) == oracle_canonical(og)


def test_simplify_on_a_loop_a_line_and_a_two_cycle():
    """by hand, k = 3.  Node 0 = AAA with the loop AAA -A-> AAA alone: one way in, one way out, the same edge: loop and node go.
    Nodes 1, 2, 3 = CCA, CAG, AGT in a line CCA -G-> CAG -T-> AGT: node 2 goes and the two edges become CCA -GT-> AGT; nodes 1 and
    3 have one edge each and stay.  Nodes 4, 5 = ACA, CAC with ACA -C-> CAC and CAC -A-> ACA, entered by nothing else: node 4
    merges its two edges into the loop CAC -AC-> CAC, node 5 then has that loop alone and goes with it.  Node 6 = TTT has no edge
    and goes."""
    nodes = ["AAA", "CCA", "CAG", "AGT", "ACA", "CAC", "TTT"]
    edges = [(0, 0, "A"), (1, 2, "G"), (2, 3, "T"), (4, 5, "C"), (5, 4, "A")]
    assert F.content(*F.simplify(nodes, edges)) == (["AGT", "CCA"], [("CCA", "AGT", "GT")])


# ---- the restatements on these structures, by hand -----------------------------------------------------------------------------

def test_spans_over_a_self_loop():
    """k = 4, letters A and C only, so that the reverse strand is off the graph.  Nodes n0 = AACC, n1 = CAAA, n2 = CCCC.  Edges:
    a = n1 -> n0, path CAAACC (len 2, window AAAC); the loop m = n0 -> n0, path AACCACAACC (len 6, windows ACCA CCAC CACA ACAA CAAC);
    b = n0 -> n2, path AACCCC (len 2, window ACCC).  The read CAAACC ACAACC ACAACC CC goes in by a, twice round m, out by b.  Its
    node windows: 2 (a, m), 8 (m, m), 14 (m, b).  The crossing at 2 has i = 2 - len_a = 0: open.  At 8, i = 8 - 6 = 2 is a crossing
    that leaves by m and windows 3..7 lie on m at 1..5: the span (a, m, m).  At 14, i = 8: the span (m, m, b).  A loop is its own
    in-edge and out-edge and is spanned like any other edge."""
    nodes = ["AACC", "CAAA", "CCCC"]
    a, m, b = 0, 1, 2
    edges = [(1, 0, "CC"), (0, 0, "ACAACC"), (0, 2, "CC")]
    spans, st = thread_spans(4, nodes, edges, ["CAAACC" + "ACAACC" * 2 + "CC"])
    assert spans == {(a, m, m): 1, (m, m, b): 1}
    assert st == dict(records=1, crossings=3, spans=2, interrupted=0, open=1)


def test_spans_over_a_self_twin_edge():
    """k = 4.  m runs from u = AACA to rc(u) = TGTT with the path AACATGTT, which is its own reverse complement (windows ACAT, the
    palindrome CATG, ATGT).  a = CCAA -> u, path CCAACA (window CAAC); its twin b = TGTT -> TTGG, path TGTTGG (window GTTG).  The read
    CCAACATGTTGG is its own reverse complement: each strand crosses u at window 2 by (a, m), open (i = 0), and rc(u) at window 6 by
    (m, b), where i = 6 - 4 = 2 is the crossing that leaves by m and 3..5 lie on m at 1..3: the span (a, m, b).  The triple is its
    own twin image (twin b, twin m, twin a) and both strands count it: 2, as the rule's twin clause gives for every triple."""
    nodes = ["AACA", "TGTT", "CCAA", "TTGG"]
    a, m, b = 0, 1, 2
    edges = [(2, 0, "CA"), (0, 1, "TGTT"), (1, 3, "GG")]
    read = "CCAACATGTTGG"
    assert R.rev_comp(read) == read and classify("AACATGTT") == "self_twin"
    spans, st = thread_spans(4, nodes, edges, [read])
    assert spans == {(a, m, b): 2}
    assert st == dict(records=1, crossings=4, spans=2, interrupted=0, open=2)


def test_a_pair_on_an_edge_and_its_twin():
    """k = 4.  e = AACA -> CACC, path AACACC (len 2, window ACAC at 1); its twin t = GGTG -> TGTT, path GGTGTT (window GTGT at 1).
    The fragment ACAC TTT GTGT reads e and then t on ONE strand, as an inverted repeat does: mate 1 starts with ACAC, and mate 2,
    the fragment's reverse complement ACAC AAA GTGT, with ACAC too.  Orientation 0: P1 = getAll(ACAC) = (e, 1), P2 =
    getAll(rc(ACAC) = GTGT) = (t, 1).  Orientation 1 is the same two lookups.  Links: both orientations give (e, t) with u = (2 + 4 -
    1) + (1 + 4) = 10, so count 2 and sum_u 20 on a link that is its own twin image (twin t, twin e).  Distances: e != t, `apart`
    twice."""
    k = 4
    index, lens = index_graph(k, [("AACA", "CC"), ("GGTG", "TT")])
    e, t = 0, 1
    frag = "ACAC" + "TTT" + "GTGT"
    pair = [frag, R.rev_comp(frag)]
    links, cls = pair_links(k, index, lens, pair, 1, 0, 4095)
    assert links == {(e, t): [2, 20]} and cls["linked"] == 2 and cls["orientations"] == 2
    hist, cls = pair_distances(k, index, lens, pair, 1, 32)
    assert cls["apart"] == 2 and cls["orientations"] == 2 and sum(hist) == 0


def test_coverage_of_a_self_twin_edge_and_its_palindromic_window():
    """k = 4, the edge AACA -> TGTT with the path AACATGTT.  Its five windows are AACA, ACAT, CATG, ATGT, TGTT: the first and the last
    are one stored k-mer, so are the second and the fourth, and CATG is its own reverse complement and stored once.  With the
    stored counts 3, 5 and 7 the edge reads 3 + 5 + 7 + 5 + 3 = 23 over 5 windows, min 3, max 7: the palindrome counts once, not
    twice, and both ends count."""
    counts = T.canonical_counts([("AACA", 3), ("ACAT", 5), ("CATG", 7)])
    assert len(counts) == 3
    cov, missing = T.coverage(counts, [("AACA", "TGTT", "TGTT")])
    assert cov == [(5, 23, 3, 7)] and missing == 0
    assert T.strand_closed([("AACA", "TGTT", "TGTT")])
