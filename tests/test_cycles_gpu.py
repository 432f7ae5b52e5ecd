"""gk_graph_build_cycles and gk_graph_simplify_keep_cycles against the plain-Python restatement (tests/cycles_ref.py), on the
cases of tests/cycles_cases.py at every key form: both unitig constructions, grids of 1 and 3 workgroups, a table of verbatim
keys; the plain build untouched beside it; the keeping simplify; and what reads a graph downstream on a circular genome."""
import numpy as np
import pytest

import cycles_cases as CC
import cycles_ref as CR
from genome_amd import dna
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.graph import CYCLE_BUILD_STATS, CYCLE_SIMPLIFY_STATS, buildGraph, loadGraph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    for name, off in (("graph_unitigs", 0), ("test_max_grid", 0)):
        c.set_option(name, off)
    c.close()


_REF = {}


def reference(name, k):
    """(table, strong, edit) of a case, computed once"""
    if (name, k) not in _REF:
        table, strong = CC.table_of(name, k)
        _REF[(name, k)] = (table, strong, CR.build_edit(table))
    return _REF[(name, k)]


def fill(ctx, k, table, strong=(), verbatim=False):
    m = HipDNAMap(ctx, k, 2 * len(table) + 64)
    if verbatim:
        m.update_inc(table)                                 # keys as they appear: either strand of any k-mer ("dirty")
    else:
        m.count_reads(dna.reads_to_bin(table), len(table))  # one read per k-mer: the hash rule picks the stored strand
    for _ in range(2 if strong else 0):
        if verbatim:
            m.update_inc(strong)
        else:
            m.count_reads(dna.reads_to_bin(strong), len(strong))
    return m


def minus(canon, edit_nodes, edit_edges):
    nodes, edges = canon
    dn, de = set(edit_nodes), set(edit_edges)
    return [n for n in nodes if n not in dn], [e for e in edges if e not in de]


@pytest.mark.parametrize("k", CC.KS)
@pytest.mark.parametrize("name", CC.BUILD_CASES)
def test_build_cycles_equals_restatement(ctx, name, k):
    table, _, (en, ee, est) = reference(name, k)
    m = fill(ctx, k, table)
    plain = buildGraph(k, m)
    plain_canon, plain_sum, plain_fp = plain.canonical(), plain.checksum(), plain.idFingerprint()
    plain.close()
    want = CR.merged(plain_canon, (en, ee))
    configs = [("graph_unitigs", 1), ("graph_unitigs", 2), ("test_max_grid", 1), ("test_max_grid", 3)]
    for opt, val in configs:
        ctx.set_option(opt, val)
        try:
            g = buildGraph(k, m, keep_cycles=True)
        finally:
            ctx.set_option(opt, 0)
        got = g.canonical()
        assert got == want, (opt, val)
        assert g.cycleStats() == est, (opt, val)
        assert tuple(g.cycleStats()) == CYCLE_BUILD_STATS
        assert g.counts() == (len(want[0]), len(want[1]), sum(len(e[2]) for e in want[1]))
        assert minus(got, en, ee) == plain_canon
        if not en:
            assert (g.checksum(), g.idFingerprint()) == (plain_sum, plain_fp), "no members: the identical graph"
        g.close()
    m.close()
    # the same k-mers stored as they appear, either strand
    m = fill(ctx, k, table, verbatim=True)
    for grid in (0, 1):
        ctx.set_option("test_max_grid", grid)
        try:
            g = buildGraph(k, m, keep_cycles=True)
        finally:
            ctx.set_option("test_max_grid", 0)
        assert g.canonical() == want and g.cycleStats() == est, grid
        g.close()
    m.close()


def test_default_is_unchanged(ctx):
    table, _, (en, _, _) = reference("circular", 31)
    m = fill(ctx, 31, table)
    g = buildGraph(31, m)
    assert g.counts() == (0, 0, 0) and g.cycleStats() is None and en
    assert g.simplifyGraph() is None
    g.close(); m.close()


def _kept(g):
    """simplifyGraph(keep_cycles=True) against the restatement applied to the graph as it was; -> the stats"""
    before = g.canonical()
    want, wst = CR.simplify_keep(*before)
    st = g.simplifyGraph(keep_cycles=True)
    assert tuple(st) == CYCLE_SIMPLIFY_STATS
    assert g.canonical() == want
    assert st == wst
    return st


@pytest.mark.parametrize("k", CC.KS)
def test_keep_one_tip_after_clip(ctx, k):
    """a circular genome whose only blemish is one tip: after clipTips the junction has one way in and one way out, the same edge"""
    table, strong, _ = reference("one_tip", k)
    m = fill(ctx, k, table, strong)
    g, g2 = buildGraph(k, m, keep_cycles=True), buildGraph(k, m)
    assert g.canonical() == g2.canonical() and g.cycleStats()["cycle_kmers"] == 0, "the tip breaks the cycle: nothing to add"
    assert g.clipTips(m) == 2 and g2.clipTips(m) == 2          # the tip and its twin
    g2.simplifyGraph()
    assert g2.counts() == (0, 0, 0), "the plain simplify deletes the replicon"
    st = _kept(g)
    nodes, edges = g.canonical()
    circ = CC.make("one_tip", k)[0][0]
    assert st["kept_self_loops"] == len(nodes) == len(edges) and len(nodes) in (1, 2)
    for s, t, seq in edges:                                    # the genome (or its reverse complement), rotated to the junction
        assert s == t and len(seq) == len(circ)
        assert s + seq[:-k] in (circ + circ) or s + seq[:-k] in CR.rc(circ + circ)
    again = g.canonical()
    assert _kept(g)["nodes_removed"] == 0 and g.canonical() == again
    g.close(); g2.close(); m.close()


@pytest.mark.parametrize("k", CC.KS)
def test_keep_popped_bubble_cycle(ctx, k):
    """bubbles popped on a circular genome leave a cycle of many merge-away nodes: one self-loop per strand survives"""
    table, strong, _ = reference("bubbles", k)
    m = fill(ctx, k, table, strong)
    g = buildGraph(k, m, keep_cycles=True)
    removed, _ = g.popBubbles(m, max_len=4 * k)
    assert removed > 0
    before_nodes = g.counts()[0]
    st = _kept(g)
    assert st["cycles_merged"] >= 1 and st["anchors_kept"] >= 1 and before_nodes > g.counts()[0] > 0
    circ = CC.make("bubbles", k)[0][0]
    loops = [e for e in g.canonical()[1] if e[0] == e[1] and len(e[2]) == len(circ)]
    assert loops, "the replicon as a self-loop"
    again = g.canonical()
    assert _kept(g)["nodes_removed"] == 0 and g.canonical() == again
    g.close(); m.close()


@pytest.mark.parametrize("k", (11, 31, 35))
def test_keep_two_anchor_cycle_is_idempotent(ctx, k):
    table, _, (en, ee, est) = reference("atat", k)
    assert est["anchors"] == 2
    m = fill(ctx, k, table)
    g = buildGraph(k, m, keep_cycles=True)
    first = g.canonical()
    for _ in range(2):
        st = _kept(g)
        assert g.canonical() == first and st == {"kept_self_loops": 0, "cycles_merged": 0, "anchors_kept": 2, "nodes_removed": 0}
    g.close(); m.close()


@pytest.mark.parametrize("k", CC.KS)
def test_keep_equals_plain_without_cycles(ctx, k):
    table, _, _ = reference("no_cycles", k)
    m = fill(ctx, k, table)
    a, b = buildGraph(k, m), buildGraph(k, m)
    a.removeBubbles(); b.removeBubbles()
    a.simplifyGraph()
    st = b.simplifyGraph(keep_cycles=True)
    assert st["kept_self_loops"] == st["cycles_merged"] == st["anchors_kept"] == 0
    assert a.checksum() == b.checksum() and a.idFingerprint() == b.idFingerprint() and a.counts() == b.counts()
    a.close(); b.close(); m.close()


def test_downstream_on_a_circular_genome(ctx, tmp_path):
    k = 31
    table, _, (en, ee, est) = reference("circular", k)
    L_ = len(CC.make("circular", k)[0][0])
    m = fill(ctx, k, table)
    g = buildGraph(k, m, keep_cycles=True)
    assert g.counts() == (2, 2, 2 * L_) and est["longest"] == L_
    assert g.edgeTwins()[2]["missing"] == 0
    c = g.contigs()
    recs = [r for r in c.text().decode().split(">") if r]
    assert len(recs) == 1 and len("".join(recs[0].split("\n")[1:])) == L_ + k
    c.close()
    p = g.gfa()
    lines = p.text().decode().splitlines()
    segs, links = [x for x in lines if x.startswith("S\t")], [x for x in lines if x.startswith("L\t")]
    assert len(segs) == 1 and links and all(x.split("\t")[1] == x.split("\t")[3] for x in links)
    p.close()
    cov = g.edgeCoverage(m)
    assert cov["missing"] == 0 and [int(x) for x in cov["kmers"]] == [L_ + 1, L_ + 1]
    g.save(tmp_path / "c.gkg")
    h = loadGraph(ctx, tmp_path / "c.gkg")
    assert h.checksum() == g.checksum() and h.canonical() == g.canonical()
    h.close(); g.close(); m.close()
