"""gk_graph_contig_stats at every level of its radix select that a test can reach: graphs with planted edge lengths
(tests/contig_stats_cases.py: what each case is for, and tests/test_contig_stats_cpu.py: the proof that it has that property)
against the plain restatement tests/checkgraph_ref.py.  Every comparison is of exact integers, all five numbers.  -m gpu.

The lengths are a condition, not a hope: every graph's live edges are read back by id (gk_graph_edges_by_id, another kernel) and
their multiset must be every target exactly twice before any statistic is looked at.

Still unpinned: the select's fourth pass and beyond (shift >= 24).  It needs an edge of 2^24 bases, which no test of a few seconds
can build; the passes at shift 0, 8 and 16, prefixes of one and two bytes and every start level up to 16 are what is held here.
"""
import ctypes as C

import numpy as np
import pytest

import checkgraph_ref as ref
import contig_stats_cases as S
from genome_amd import _lib as L
from genome_amd import dna
from genome_amd.dnamap import HipDNAMap
from genome_amd.graph import buildGraph
from test_checkgraph_host_gpu import CHECK, run
from test_small_grid_gpu import capped
from test_variants_gpu import ctx  # noqa: F401 (the module-scoped context fixture)

pytestmark = pytest.mark.gpu
RUNS = [(name, 31) for name in S.CASES] + [(name, 47) for name in ("three_level",) + S.BOUNDARY_256]


def live_lengths(graph):
    """the live edges' lengths by the by-id reads, sorted, and the ids they belong to"""
    _, bound = graph.idBounds()
    info = graph.edgesById(np.arange(bound, dtype=np.uint32))
    ids = np.flatnonzero(info["alive"])
    order = np.argsort(info["len"][ids], kind="stable")
    return [int(x) for x in info["len"][ids][order]], ids[order]


class Planted:
    """the graph of a case's reads: count -> buildGraph -> simplifyGraph; its lengths are the planted ones or the test fails"""

    def __init__(self, ctx, name, k):
        reads = S.all_reads(name, k)
        self.m = HipDNAMap(ctx, k)
        self.m.count_reads(dna.reads_to_bin(reads), len(reads))
        self.graph = buildGraph(k, self.m)
        self.graph.simplifyGraph()
        self.lengths, _ = live_lengths(self.graph)
        assert self.lengths == S.lengths_of(name), f"{name}, k = {k}: the graph does not hold the planted lengths"

    def close(self):
        self.graph.close(); self.m.close()


@pytest.fixture(scope="module")
def planted(ctx):  # noqa: F811
    made = {}

    def get(name, k, fresh=False):
        """fresh: a graph of the caller's own to edit, closed by the caller"""
        if fresh:
            return Planted(ctx, name, k)
        if (name, k) not in made:
            made[(name, k)] = Planted(ctx, name, k)
        return made[(name, k)]

    yield get
    for p in made.values():
        p.close()


def check_stats(graph, lengths):
    """all five numbers at every cutoff the lengths call for (contig_stats_cases.cutoffs); nothing remains at the maximum"""
    for cutoff in S.cutoffs(lengths):
        assert graph.contigStats(cutoff) == ref.contig_stats(lengths, cutoff), cutoff
    assert graph.contigStats(max(lengths)) == S.ZERO and graph.contigStats(max(lengths) - 1)["count"] == lengths.count(max(lengths))


@pytest.mark.parametrize("name,k", RUNS)
def test_the_five_numbers(planted, name, k):
    p = planted(name, k)
    check_stats(p.graph, p.lengths)


@pytest.mark.parametrize("name", ["three_level", "two_level_split"])
def test_one_workgroup(ctx, planted, name):  # noqa: F811
    """the same graph with every launch capped to one workgroup: one workgroup's LDS histogram takes every length"""
    p = planted(name, 31)
    with capped(ctx, 1):
        check_stats(p.graph, p.lengths)
        under_cap = [p.graph.contigStats(c) for c in S.cutoffs(p.lengths)]
    assert under_cap == [p.graph.contigStats(c) for c in S.cutoffs(p.lengths)]


def test_dead_edges(planted):
    """three_level without its longest edges, step by step on the same arrays: the maximum falls to 65 537 (the N50 stays at
    65 536), then to 65 536 (the N50 moves below the byte boundary, to 65 535, under a maximum of three bytes), then to 65 535 (the
    select starts one level lower)"""
    p = planted("three_level", 31, fresh=True)
    try:
        left = list(p.lengths)
        for gone, want_max, want_n50 in ((70000, 65537, 65536), (65537, 65536, 65535), (65536, 65535, 65535)):
            lengths, ids = live_lengths(p.graph)
            assert p.graph.removeEdgesById(ids[np.array(lengths) == gone]) == 2
            left = [x for x in left if x != gone]
            assert live_lengths(p.graph)[0] == left
            check_stats(p.graph, left)
            got = p.graph.contigStats(0)
            assert (got["max"], got["n50"], got["count"]) == (want_max, want_n50, len(left))
    finally:
        p.close()


@pytest.mark.parametrize("name", ["three_level", "two_level_split"])
def test_null_outputs(ctx, planted, name):  # noqa: F811
    """a raw call that asks for the median alone, and one for the N50 alone"""
    p = planted(name, 31)
    for cutoff in (0, min(p.lengths)):
        want = ref.contig_stats(p.lengths, cutoff)
        for slot, key in ((2, "median"), (3, "n50")):
            v = C.c_uint64(12345)
            args = [None] * 5
            args[slot] = C.byref(v)
            L.check(L.lib().gk_graph_contig_stats(p.graph.h, cutoff, *args), ctx.h)
            assert v.value == want[key], (cutoff, key)


def test_the_host_tool(planted, tmp_path):
    """check_graph on the saved three_level graph: its "contigs" object is the restatement's"""
    p = planted("three_level", 31)
    p.graph.save(tmp_path / "g.gkg")
    (tmp_path / "ref.fasta").write_text(">c\n" + S.chromosomes("three_level", 31)[0] + "\n")
    got = run([CHECK, tmp_path / "g.gkg", tmp_path / "ref.fasta", "--longer-than", 100])
    want = ref.contig_stats(p.lengths, 100)
    assert got["contigs"] == want and 0 < want["count"] < len(p.lengths) and want["median"] < 256 < want["n50"]
    assert got["missing"] == 0 and got["windows"] > 0
