"""The restatement of GraphBuilder.scala:37-54 (tests/components_ref.py) against hand-written graphs, and against the oracle's
components and retainLargest on graphs of reads.  No GPU."""
import pytest

from genome_amd import dna
from genome_amd.dna import rev_complement as rc
from oracle import oracle as O

import components_ref as CR
from test_fuzz_gpu import _oracle_graph
from test_variants_gpu import _cc_reads, _component_sizes


def test_the_order_is_the_oracles():
    # the last base weighs most, A < G < C < T; beyond 32 bases the high word decides
    assert sorted(["TA", "AG", "GG", "CA", "AC"], key=CR.kmer_key) == ["CA", "TA", "AG", "GG", "AC"]
    a, b = "T" * 32 + "A", "A" * 32 + "G"
    assert CR.kmer_key(a) < CR.kmer_key(b) and CR.kmer_key(a) == (0, 2 ** 64 - 1)
    for s in ("AGCT", "TTTTG", "C" * 33 + "T", "AG" * 32):
        hi, lo = CR.kmer_key(s)
        assert (lo, hi) == dna.pack(s) and CR.kmer_key(rc(rc(s))) == (hi, lo)


def test_empty_graph():
    assert CR.components([], []) == [] and CR.stats([], []) == []
    assert CR.histograms([], []) == ([], []) and CR.retained([], []) == ([], []) and CR.tied_for_largest([], []) == []


def test_singleton_node_and_self_loop():
    # a node without edges is a component of one node and length 0; a self-loop adds its length and joins nothing
    nodes = ["AAG", "CCT", "GGA"]
    edges = [("CCT", "CCT", "ACCT")]
    assert CR.stats(nodes, edges) == [(1, 0), (1, 0), (1, 4)]
    assert CR.histograms(nodes, edges) == ([(1, 3)], [(0, 2), (4, 1)])
    # three components tied at one node: the smallest k-mer is GGA (last base A; then G < C in the middle)
    assert sorted(CR.kmer_key(s) for s in nodes)[0] == CR.kmer_key("GGA")
    assert CR.retained(nodes, edges) == (["GGA"], [])
    assert CR.retained(["AAG", "CCT"], edges) == (["AAG"], [])           # last base G < T: the self-loop's node goes, and its edge


def test_two_components_tied_in_size_and_an_edge_inside_one_component():
    # X: AAA -> AAG -> AGC, and AAA -> AGC directly (start and end already joined: the component count stays, the length grows)
    # Y: TTT -> TTC -> TCA, one edge fewer
    nodes = ["AAA", "AAG", "AGC", "TTT", "TTC", "TCA"]
    ex = [("AAA", "AAG", "G"), ("AAG", "AGC", "C"), ("AAA", "AGC", "CAGC")]
    ey = [("TTT", "TTC", "C"), ("TTC", "TCA", "A")]
    comps = CR.components(nodes, ex + ey)
    assert sorted((n, ln) for _m, n, ln in comps) == [(3, 2), (3, 6)]
    assert CR.histograms(nodes, ex + ey) == ([(3, 2)], [(2, 1), (6, 1)])
    assert sorted(map(tuple, CR.tied_for_largest(nodes, ex + ey))) == [("AAA", "AAG", "AGC"), ("TCA", "TTC", "TTT")]
    # the tie goes to the component holding the smallest k-mer: AAA
    assert CR.retained(nodes, ex + ey) == (["AAA", "AAG", "AGC"], ex)
    # without AAA's component's claim to it: rename AAA -> CAT; now TCA (last base A) is the smallest of all
    ren = lambda s: "CAT" if s == "AAA" else s
    nodes2 = [ren(s) for s in nodes]
    ex2 = [(ren(a), ren(b), q) for a, b, q in ex]
    assert CR.retained(nodes2, ex2 + ey) == (["TTT", "TTC", "TCA"], ey)
    # a larger component wins whatever it holds
    assert CR.retained(nodes2 + ["TTG"], ex2 + ey + [("TTT", "TTG", "G")])[0] == ["TTT", "TTC", "TCA", "TTG"]
    # the length is counted where an edge STARTS: an edge is never split between two components
    assert CR.stats(["AAA", "AAG"], [("AAA", "AAG", "GGGGG")]) == [(2, 5)]


def test_a_node_given_twice_is_refused():
    with pytest.raises(AssertionError):
        CR.components(["AAA", "AAA"], [])


@pytest.mark.parametrize("shape", ["equal", "path", "cycle", "singletons"])
@pytest.mark.parametrize("k", [15, 31, 47])
def test_against_the_oracle_on_graphs_of_reads(k, shape):
    """node counts as the union-find of tests/test_variants_gpu.py has them, the number of components and the retained graph as
    the oracle has them; "equal" is 48 components of one size, so the tie rule decides there"""
    reads = _cc_reads(k, shape)
    ref = O.PMap(k, 1)
    ref.count_reads(dna.reads_to_bin(reads), len(reads))
    ref.delete_lt(2 if shape == "singletons" else 1)
    og = O.Graph(ref)
    nodes, edges = _oracle_graph(og, k)
    assert nodes == sorted(nodes, key=CR.kmer_key)           # the oracle numbers its nodes in ascending k-mer order: this order
    st = CR.stats(nodes, edges)
    assert sorted(n for n, _ln in st) == _component_sizes(og, k)
    assert len(st) == og.num_components()
    assert sum(ln for _n, ln in st) == og.total_edge_len()
    h1, h2 = CR.histograms(nodes, edges)
    assert sum(c for _v, c in h1) == sum(c for _v, c in h2) == len(st)
    if shape == "equal":
        assert len(CR.tied_for_largest(nodes, edges)) >= 24
    want_nodes, want_edges = CR.retained(nodes, edges)
    assert og.retain_largest() == len(want_nodes)
    assert _oracle_graph(og, k) == (want_nodes, want_edges)
    og.close(); ref.close()
