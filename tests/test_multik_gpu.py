"""gk_map_add_graph_paths on the device against its restatement (tests/multik_ref.py), exact: the sorted (key, count) export of the
table after the call == the export before + what the restatement adds, and the six stats (-m gpu); and genome_amd.multik.assemble on
the construction k = 55 alone cannot cross.

Every key form of graph and table, into an empty table and into one that holds the reads' counts, count and graph layout; contigs
of exactly 0, 1, 2, 15, 16, 17, 16 * 256 - 1, 16 * 256, 16 * 256 + 1 windows as single-edge graphs (k2 = k1 + 1 puts the first
windows across the seam of node k-mer and edge bases); chunks of 16, 17 and 1000 windows and launch grids of 1 and 3 workgroups;
dead edges, a reverse edge whose twin is dead, a self_twin edge, the folded graphs, graphs after simplifyGraph, after a split by
support and with node copies that share a k-mer; a table that must grow several times; the errors.
"""
import ctypes as C
import random

import numpy as np
import pytest

from genome_amd import _lib as L
from genome_amd import dna
from genome_amd.dnamap import GRAPH_PATHS_STATS, Context, HipDNAMap
from genome_amd.graph import Support, buildGraph
from genome_amd.multik import assemble
from oracle import pyref as R

import contigs_ref as CR
import folded_cases as FC
import multik_cases as MC
import multik_ref as MR
import test_edge_coverage_gpu as EC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def rows(m):
    lo, hi, cnt = m.sorted_items()
    return list(zip(hi.tolist(), lo.tolist(), cnt.tolist()))


def seed_and_compare(g, dst, weight=3):
    """dst.add_graph_paths(g, weight): stats and table == the restatement's; the graph is as it was -> the stats"""
    edges = g.canonical()[1]
    added, want = MR.add_graph_paths(edges, dst.k, weight)
    before = rows(dst)
    fp, chk = g.idFingerprint(), g.checksum()
    got = dst.add_graph_paths(g, weight)
    assert tuple(got) == GRAPH_PATHS_STATS == MR.STATS
    assert got == want
    assert got["live_edges"] == got["short"] + got["forward"] + got["self_twin"] + got["reverse"] == g.counts()[1]
    assert rows(dst) == MR.merged(before, added)
    assert dst.verify()[1] == 0
    assert (g.idFingerprint(), g.checksum()) == (fp, chk)
    return got


def graph_of_reads(ctx, k, reads, min_count=1):
    m = HipDNAMap(ctx, k)
    m.count_reads(dna.reads_to_bin(reads), len(reads))
    if min_count > 1:
        m.deleteAll_lt(min_count)
    return m, buildGraph(k, m)


def bubble_reads(k1, n=300, seed=3):
    """tiles of a random sequence and of its copy with one substitution: a bubble between two flanks, and all their twins"""
    rnd = random.Random(100 * seed + k1)
    s = MC.rand_seq(rnd, n)
    t = s[:n // 2] + [b for b in "AGCT" if b != s[n // 2]][0] + s[n // 2 + 1:]
    return [x[i:i + 100] for x in (s, t) for i in range(0, n - 100 + 1, 5)]


KEY_FORMS = [(11, 15), (21, 31), (31, 34), (21, 55), (31, 64), (34, 35), (40, 64)]


@pytest.mark.parametrize("k1,k2", KEY_FORMS)
def test_every_key_form_layout_and_prefill(ctx, k1, k2):
    reads = bubble_reads(k1)
    m1, g = graph_of_reads(ctx, k1, reads)
    assert g.counts()[1] >= 6
    for for_graph in (False, True):
        for prefill in (False, True):
            dst = HipDNAMap(ctx, k2, 4096, for_graph=for_graph)
            if for_graph and k2 <= 31:
                assert dst.stats()["slot_bytes"] == 16
            if prefill:
                dst.count_reads(dna.reads_to_bin(reads), len(reads))
                assert dst.size() > 0
            st = seed_and_compare(g, dst, weight=3 if prefill else 65535)
            assert st["forward"] == st["reverse"] >= 2 and st["windows"] > 0
            dst.close()
    g.close(); m1.close()


WINDOWS = (0, 1, 2, 15, 16, 17, 16 * 256 - 1, 16 * 256, 16 * 256 + 1)


@pytest.mark.parametrize("k1,k2", [(21, 22), (21, 23), (21, 24), (31, 34), (21, 55), (34, 35), (40, 64)])
def test_window_and_run_edges(ctx, k1, k2):
    """single-edge graphs of planted linear genomes: n = k2 - 1 + windows bases"""
    for w in WINDOWS:
        n = k2 - 1 + w
        s = MC.linear_genome(k1, n, 7 * k1 + k2)
        counts = {R.canon(s[i:i + k1]): 2 for i in range(n - k1 + 1)}
        m1 = EC.fill(ctx, k1, counts)
        g = buildGraph(k1, m1)
        edges = g.canonical()[1]
        lone = n == k1                                           # (k2 = k1 + 1, no window: one isolated k-mer, a graph without an edge)
        assert sorted(a + q for a, _b, q in edges) == ([] if lone else sorted((s, R.rev_comp(s))))
        dst = HipDNAMap(ctx, k2, 64)
        st = seed_and_compare(g, dst, weight=5)
        assert st["windows"] == w and st["short"] == (2 if w == 0 and not lone else 0) and st["forward"] == st["reverse"] == (1 if w else 0)
        assert ctx.multik_chunks() == (1 if w else 0)
        dst.close(); g.close(); m1.close()


@pytest.mark.parametrize("chunk", [16, 17, 1000])
def test_chunks(ctx, chunk):
    k1, k2 = 21, 31
    m1, g = graph_of_reads(ctx, k1, bubble_reads(k1, n=3000))
    ctx.set_option("test_multik_chunk_windows", chunk)
    try:
        dst = HipDNAMap(ctx, k2, 64)
        st = seed_and_compare(g, dst)
        assert st["windows"] > 2000
        per = max(1, chunk // 16)
        runs = sum((len(a + q) - k2 + 1 + 15) // 16 for a, _b, q in g.canonical()[1] if CR.classify(a + q, k2) in ("forward", "self_twin"))
        assert ctx.multik_chunks() == (runs + per - 1) // per > 1
        dst.close()
    finally:
        ctx.set_option("test_multik_chunk_windows", 0)
    g.close(); m1.close()


@pytest.mark.parametrize("grid", [1, 3])
def test_small_launch_grids(ctx, grid):
    k1, k2 = 21, 55
    m1, g = graph_of_reads(ctx, k1, bubble_reads(k1, n=16000))
    ctx.set_option("test_max_grid", grid)
    try:
        uses = ctx.grid_cap_uses()
        dst = HipDNAMap(ctx, k2, 64)
        st = seed_and_compare(g, dst)
        assert ctx.grid_cap_uses() > uses and st["windows"] > 16 * 256 * 3       # every lane of every workgroup takes several runs
        dst.close()
    finally:
        ctx.set_option("test_max_grid", 0)
    g.close(); m1.close()


def test_dead_edges_and_a_reverse_edge_without_its_twin(ctx):
    k1, k2 = 21, 24
    m1, g = graph_of_reads(ctx, k1, bubble_reads(k1))
    edges, ids = EC.edges_with_ids(g)
    cls = [CR.classify(a + q, k2) for a, _b, q in edges]
    fwd = [i for i, c in zip(ids, cls) if c == "forward"]
    rev = [i for i, c in zip(ids, cls) if c == "reverse"]
    assert len(fwd) == len(rev) >= 3
    # a reverse edge goes: its forward twin is still added; a forward edge goes: its reverse twin stays and is not added
    path = {i: a + q for (a, _b, q), i in zip(edges, ids)}
    twin_of_first = [i for i in rev if path[i] == R.rev_comp(path[fwd[0]])]
    assert len(twin_of_first) == 1
    assert g.removeEdgesById([twin_of_first[0], fwd[1]]) == 2
    dst = HipDNAMap(ctx, k2, 64)
    st = seed_and_compare(g, dst)
    assert st["forward"] == len(fwd) - 1 == st["reverse"] and st["live_edges"] == len(ids) - 2
    gone = [e for e, i in zip(edges, ids) if i == fwd[1]][0]
    p = gone[0] + gone[2]
    inner = R.canon(p[len(p) // 2 - k2 // 2:][:k2])          # a window of the dead forward edge: in no other contig
    assert dst.apply(inner) is None
    # every edge dead: zeros, the table as it was
    g.removeEdgesById(np.arange(g.idBounds()[1], dtype=np.uint32))
    before = rows(dst)
    assert dst.add_graph_paths(g, 3) == dict.fromkeys(GRAPH_PATHS_STATS, 0) and rows(dst) == before
    dst.close(); g.close(); m1.close()


@pytest.mark.parametrize("k1,k2", [(21, 22), (21, 23), (34, 36)])
def test_self_twin_edge(ctx, k1, k2):
    """X ++ rc(X): its mirrored windows count twice; at even k2 the middle window is a palindrome and counts once"""
    x = MC.rand_seq(random.Random(9 * k1), 60)
    s = x + R.rev_comp(x)
    counts = {R.canon(s[i:i + k1]): 4 for i in range(len(s) - k1 + 1)}
    m1 = EC.fill(ctx, k1, counts)
    g = buildGraph(k1, m1)
    dst = HipDNAMap(ctx, k2, 64)
    st = seed_and_compare(g, dst, weight=7)
    assert st["self_twin"] >= 1
    if g.counts()[1] == 1:
        mid = s[60 - k2 // 2:][:k2]
        assert dst.apply(R.canon(s[:k2])) == 14 and dst.apply(R.canon(mid)) == (7 if k2 % 2 == 0 else 14)
    dst.close(); g.close(); m1.close()


@pytest.mark.parametrize("k1", [11, 12, 34])
def test_folded_graphs_simplified_and_split(ctx, k1):
    c = FC.case(k1, FC.SEEDS[k1], "clean")
    k2 = k1 + 2
    m1, g = graph_of_reads(ctx, k1, c.graph_reads, c.min_count)
    dst = HipDNAMap(ctx, k2, 64)
    st = seed_and_compare(g, dst)
    assert st["self_twin"] >= 1 and st["short"] >= 1 and st["forward"] == st["reverse"]
    g.simplifyGraph()
    seed_and_compare(g, dst)
    # a split by the support of threaded reads: node copies that share a k-mer (point edits: test_node_copies_that_share_a_kmer)
    vm = g.getGraphMap()
    sup = Support(ctx)
    g.threadReads(vm, sup, (dna.reads_to_bin(c.singles), len(c.singles)))
    g.splitBySupport(sup, 1)
    seed_and_compare(g, dst)
    sup.close(); vm.close(); dst.close(); g.close(); m1.close()


def test_node_copies_that_share_a_kmer(ctx):
    k1, k2 = 31, 34
    m1, g = graph_of_reads(ctx, k1, bubble_reads(k1))
    named = EC.edges_with_ids(g)
    (_s0, e0, _q0), (s1, _e1, _q1) = named[0][0], named[0][1]
    g.replaceEnd(named[1][0], g.addNode(e0))
    g.replaceStart(named[1][1], g.addNode(s1))
    dst = HipDNAMap(ctx, k2, 64)
    seed_and_compare(g, dst)
    dst.close(); g.close(); m1.close()


def test_a_table_that_must_grow(ctx):
    k1, k2 = 21, 31
    m1, g = graph_of_reads(ctx, k1, bubble_reads(k1, n=8000))
    # (the insert reserves room for a whole chunk before it runs: small chunks let the table grow step by step)
    ctx.set_option("test_multik_chunk_windows", 1024)
    try:
        dst = HipDNAMap(ctx, k2, 16)
        slots, grows = dst.slots(), dst.stats()["grows"]
        st = seed_and_compare(g, dst)
        assert st["windows"] > slots and dst.slots() > slots and dst.stats()["grows"] >= grows + 2
        dst.close()
    finally:
        ctx.set_option("test_multik_chunk_windows", 0)
    g.close(); m1.close()


def test_errors_leave_table_and_graph_alone(ctx):
    k1, k2 = 21, 31
    reads = bubble_reads(k1)
    m1, g = graph_of_reads(ctx, k1, reads)
    dst = HipDNAMap(ctx, k2, 64)
    dst.count_reads(dna.reads_to_bin(reads), len(reads))
    plan = g.contigs()
    text = plan.text()
    chk = dst.verify_checksum()
    lib = L.lib()
    st = np.full(6, 99, np.uint64)
    other_ctx = Context(0)
    foreign = HipDNAMap(other_ctx, k2, 64)
    same_k, smaller = HipDNAMap(ctx, k1, 64), HipDNAMap(ctx, k1 - 2, 64)
    for args in ((None, g.h, 3), (dst.h, None, 3), (foreign.h, g.h, 3), (same_k.h, g.h, 3), (smaller.h, g.h, 3), (dst.h, g.h, 0), (dst.h, g.h, 65536)):
        assert lib.gk_map_add_graph_paths(args[0], args[1], args[2], L.ptr(st, C.c_uint64)) == L.GK_E_INVALID, args
        assert dst.verify_checksum() == chk and plan.text() == text
    assert foreign.size() == same_k.size() == smaller.size() == 0
    with pytest.raises(L.GkError) as err:
        dst.add_graph_paths(g, 0)
    assert err.value.code == L.GK_E_INVALID
    # a call that works leaves the plan readable too: the graph's state counter does not move
    assert lib.gk_map_add_graph_paths(dst.h, g.h, 65535, None) == L.GK_OK
    assert plan.text() == text and dst.verify_checksum() != chk
    plan.close(); smaller.close(); same_k.close(); foreign.close(); other_ctx.close(); dst.close(); g.close(); m1.close()


# ---- end to end: the construction of tests/multik_cases.py --------------------------------------------------------------

@pytest.fixture(scope="module")
def dip():
    genome = MC.dip_genome()
    reads = MC.dip_reads(genome)
    return genome, dna.reads_to_bin(reads), len(reads)


def contig_records(g):
    c = g.contigs(line_width=0, strands=1)
    recs = [seq for _i, _n, _c, seq in CR.parse(c.text())]
    c.close()
    return recs


def test_k55_alone_breaks_at_the_dip(ctx, dip):
    genome, bin_bytes, n = dip
    m, g, stages = assemble(ctx, bin_bytes, n, [55])
    recs = contig_records(g)
    assert len(recs) == 2 and all(r in genome or R.rev_comp(r) in genome for r in recs)
    assert len(stages) == 1 and stages[0]["windows"] == 0 and stages[0]["distinct_before_seed"] == stages[0]["distinct_after_seed"]
    g.close(); m.close()


@pytest.mark.parametrize("ks", [[21, 55], [21, 31, 55]])
def test_seeded_k55_crosses_the_dip(ctx, dip, ks):
    genome, bin_bytes, n = dip
    m, g, stages = assemble(ctx, bin_bytes, n, ks)
    recs = contig_records(g)
    assert len(recs) == 1 and recs[0] in (genome, R.rev_comp(genome))
    assert [s["k"] for s in stages] == ks and all(s["rounds"] == 3 for s in stages)
    # every seed stage's stats are the restatement's on the graph the stage before left
    for i in range(1, len(ks)):
        pm, pg, _ = assemble(ctx, bin_bytes, n, ks[:i])
        pg.simplifyGraph()
        added, want = MR.add_graph_paths(pg.canonical()[1], ks[i], 3)
        assert {name: stages[i][name] for name in MR.STATS} == want and want["forward"] == 1 and want["windows"] == len(genome) - ks[i] + 1
        assert stages[i]["distinct_after_seed"] - stages[i]["distinct_before_seed"] == (MC.MISSING_55 if ks[i] == 55 else 0)
        pg.close(); pm.close()
    assert (stages[-1]["nodes"], stages[-1]["edges"]) == g.counts()[:2] and g.counts()[1] == 2
    g.close(); m.close()


def test_assemble_refuses_bad_ks_before_any_device_work():
    for ks in ([], [31, 21], [21, 21], [32], [21, 33], [1, 21], [21, 65], ["21"]):
        with pytest.raises(ValueError):
            assemble(None, b"", 0, ks)
