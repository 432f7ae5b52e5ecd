"""The read, pair and placement kernels on folded graphs (-m gpu): tandem and inverted repeats, a hairpin, homopolymer and two-base
cycles and, at even k, a palindromic node (tests/folded_cases.py; tests/test_folded_cpu.py shows on the CPU that every structure and
class is there).  Every comparison is exact: by content, an edge being its (start k-mer, first base), against the restatements on
the ORACLE's graph; by id (test_spans_gpu.by_id) where the copies of the span split must be told apart."""
from collections import Counter

import pytest

import folded_cases as F
import fillgaps_ref as FR
import judge_ref as J
import test_edge_coverage_gpu as EC
import test_fillgaps_gpu as FG
import test_links_gpu as LG
import test_spans_gpu as SG
from contigs_ref import classify
from genome_amd import dna
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.graph import HipSpans, Support, buildGraph, scaffoldChains
from insert_ref import index_graph, pair_distances
from links_cases import by_content
from links_ref import chains, joins, pair_links
from oracle import pyref as R
from pairs_ref import gpu_canonical, gpu_support_by_content
from thread_ref import thread_reads, twin_edges

pytestmark = pytest.mark.gpu

CASES = [(k, v) for k in F.KS for v in F.VARIANTS]


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def build(ctx, c):
    """-> (count table, graph, position map); the graph must be the oracle's: the precondition of everything else"""
    m = HipDNAMap(ctx, c.k)
    m.count_reads(dna.reads_to_bin(c.graph_reads), len(c.graph_reads))
    if c.min_count > 1:
        m.deleteAll_lt(c.min_count)
    g = buildGraph(c.k, m)
    assert gpu_canonical(g) == c.canonical()
    return m, g, g.getGraphMap()


def support_by_id(sup):
    e1, e2, cnt = sup.items()
    return Counter({(int(a), int(b)): int(n) for a, b, n in zip(e1, e2, cnt)})


def placed(p):
    """Placements.edges() as judge_ref.place gives it: {id: (class, record, pos, windows_fwd, windows_rev)}"""
    e = p.edges()
    return {i: x for i, x in enumerate(zip(e["cls"], e["record"], e["pos"], e["windows_fwd"], e["windows_rev"]))}


def compact(nodes, edges):
    """test_spans_gpu.by_id's lists without the dead ids, as the restatements take them -> (node k-mers, edges (start rank, end
    rank, sequence), the id of every edge kept)"""
    nid = [i for i, x in enumerate(nodes) if x is not None]
    eid = [i for i, x in enumerate(edges) if x is not None]
    rank = {v: i for i, v in enumerate(nid)}
    return [nodes[i] for i in nid], [(rank[edges[e][0]], rank[edges[e][1]], edges[e][2]) for e in eid], eid


def live(nodes, edges):
    """test_spans_gpu.by_id's lists -> judge_ref's dicts"""
    return {i: s for i, s in enumerate(nodes) if s is not None}, {e: (nodes[x[0]], x[2]) for e, x in enumerate(edges) if x is not None}


@pytest.mark.parametrize("k, variant", CASES)
def test_thread_reads_and_spans(ctx, k, variant):
    c = F.case(k, F.SEEDS[k], variant)
    m, g, vm = build(ctx, c)
    nodes, edges, keys = c.by_index()
    data = (dna.reads_to_bin(c.singles), len(c.singles))
    # threadReads: support by content and the seven stats
    want_sup, want = thread_reads(k, nodes, edges, c.singles)
    assert tuple(want[x] for x in F.THREAD_STATS) == F.TABLE[(k, variant)]["thread"]
    sup = Support(ctx)
    assert g.threadReads(vm, sup, data) == want
    got = gpu_support_by_content(g, k, sup)
    assert got == Counter({(keys[e], keys[f]): n for (e, f), n in want_sup.items()})
    # the symmetry the header claims, on the device's own output: count(e, f) == count(twin f, twin e)
    twin = {keys[e]: keys[t] for e, t in twin_edges(k, nodes, edges).items()}
    assert all(got[(twin[f], twin[e])] == n for (e, f), n in got.items())
    # threadSpans by id: triples and the five stats
    want_spans, want_st = SG.restate(g, c.singles)
    assert tuple(want_st[x] for x in F.SPAN_STATS) == F.TABLE[(k, variant)]["spans"]
    sp = HipSpans(ctx)
    assert g.threadSpans(vm, sp, data) == want_st and SG.table(sp) == want_spans
    # one workgroup
    uses = ctx.grid_cap_uses()
    ctx.set_option("test_max_grid", 1)
    try:
        sup1, sp1 = Support(ctx), HipSpans(ctx)
        assert g.threadReads(vm, sup1, data) == want and g.threadSpans(vm, sp1, data) == want_st
    finally:
        ctx.set_option("test_max_grid", 0)
    assert ctx.grid_cap_uses() > uses
    assert gpu_support_by_content(g, k, sup1) == got and SG.table(sp1) == want_spans
    for x in (sup, sup1, sp, sp1, vm, g, m):
        x.close()


def split_fresh(ctx, c, cutoff):
    """a fresh graph, its spans, splitEdgesBySpans at `cutoff` against the restatement by id -> (table, graph, the stats)"""
    m, g, vm = build(ctx, c)
    sp = HipSpans(ctx)
    g.threadSpans(vm, sp, (dna.reads_to_bin(c.singles), len(c.singles)))
    vm.close()
    st = SG.check_edit(g, sp, cutoff)
    assert tuple(st[x] for x in F.SPLIT_STATS) == F.TABLE[(c.k, c.variant)]["split%d" % cutoff]
    sp.close()
    paths = SG.live_paths(g)
    assert paths == sorted(R.rev_comp(p) for p in paths)                       # still strand-closed, by sequence
    return m, g, st


def simplify_and_compare(g):
    """simplifyGraph on the device == folded_cases.simplify on the graph as the device holds it now, by content"""
    want = F.content(*F.simplify(*SG.by_id(g)))
    g.simplifyGraph()
    assert gpu_canonical(g) == want
    paths = SG.live_paths(g)
    assert paths == sorted(R.rev_comp(p) for p in paths)


@pytest.mark.parametrize("k, variant", CASES)
def test_split_at_cutoff_3_then_simplify(ctx, k, variant):
    c = F.case(k, F.SEEDS[k], variant)
    m, g, st = split_fresh(ctx, c, 3)
    simplify_and_compare(g)
    g.close(); m.close()


@pytest.mark.parametrize("k, variant", CASES)
def test_split_edges_by_spans_and_the_classes_of_shared_kmers(ctx, k, variant):
    """cutoff 1 on a fresh graph; then, on the split graph, whose copies share k-mers: threadReads, pairDistances, pairLinks and
    place by id; then simplifyGraph against the same edit on the restatement's side"""
    c = F.case(k, F.SEEDS[k], variant)
    m, g, st = split_fresh(ctx, c, 1)
    if variant == "clean":
        assert st["resolved"] > 0 and st["new_edges"] > 0
        assert F.content(*SG.by_id(g)) == F.content(*F.split_graph(c, 1)[:2])           # the oracle's graph under the same edit
    nodes, edges = SG.by_id(g)
    vm = g.getGraphMap()
    cn, ce, eid = compact(nodes, edges)
    index, lens = index_graph(k, [(cn[s], q) for s, _, q in ce], nodes=cn)
    shared = sum(len(v) >= 2 for v in index.values())
    # threadReads
    want_sup, want = thread_reads(k, cn, ce, c.singles)
    want_sup = Counter({(eid[e], eid[f]): n for (e, f), n in want_sup.items()})
    assert (want["repeated"] > 0) == (shared > 0)
    sup = Support(ctx)
    assert g.threadReads(vm, sup, (dna.reads_to_bin(c.singles), len(c.singles))) == want and support_by_id(sup) == want_sup
    # pairDistances
    want_hist, want_cls = pair_distances(k, index, lens, c.pairs, c.npairs, F.BINS)
    hist, cls = g.pairDistances(vm, (dna.reads_to_bin(c.pairs), c.npairs), bins=F.BINS)
    assert cls == want_cls and hist.tolist() == want_hist
    # pairLinks
    want_links, want_cls = pair_links(k, index, lens, c.pairs, c.npairs, 0, F.LINK_SPAN + k)
    links, cls = LG.link(g, vm, c.pairs, min_len=0, max_span=F.LINK_SPAN + k)
    assert cls == want_cls and {(e, f): [n, s] for e, f, n, s in LG.records(links)} == {(eid[e], eid[f]): v for (e, f), v in want_links.items()}
    # place
    pst, pwant = J.place(k, *live(nodes, edges), [c.genome], id_bound=len(edges))
    p = g.place(vm, [c.genome])
    assert p.stats() == pst and placed(p) == pwant
    if variant == "clean":
        assert shared > 0 and want_cls["repetitive"] > 0 and pst["fwd_repetitive"] > 0 and pst["rev_repetitive"] > 0
    for x in (p, links, sup, vm):
        x.close()
    simplify_and_compare(g)
    if variant == "clean":
        assert gpu_canonical(g) == F.content(*F.simplify(*F.split_graph(c, 1)[:2]))
    g.close(); m.close()


@pytest.mark.parametrize("k, variant", CASES)
def test_pair_distances_links_joins_and_chains(ctx, k, variant):
    c = F.case(k, F.SEEDS[k], variant)
    m, g, vm = build(ctx, c)
    index, lens, okeys, _ = c.indexed()
    data = (dna.reads_to_bin(c.pairs), c.npairs)
    want_hist, want_cls = pair_distances(k, index, lens, c.pairs, c.npairs, F.BINS)
    assert tuple(want_cls[x] for x in F.INSERT_CLASSES) == F.TABLE[(k, variant)]["insert"]
    hist, cls = g.pairDistances(vm, data, bins=F.BINS)
    assert cls == want_cls and hist.tolist() == want_hist
    want_links, want_cls = pair_links(k, index, lens, c.pairs, c.npairs, 0, F.LINK_SPAN + k)
    assert tuple(want_cls[x] for x in F.LINK_CLASSES) == F.TABLE[(k, variant)]["links"]
    want_joins, want_st = joins(want_links, F.SUPPORT)
    keys = LG.edge_keys(g)
    links, cls = LG.link(g, vm, c.pairs, min_len=0, max_span=F.LINK_SPAN + k)
    assert cls == want_cls and LG.content(links, keys) == by_content(want_links, okeys)
    got_joins, st = LG.content_joins(links, keys, F.SUPPORT)
    assert st == want_st and got_joins == sorted((okeys[e], okeys[f], n, s) for e, f, n, s in want_joins)
    # the chains.  The joins above are the restatement's, by content; on the device's own join list (ids) scaffoldChains must give
    # links_ref.chains member for member, a cycle starting at its smallest id; `cycles` is the NUMBER of cycles among the chains
    (e1, e2, _, _), _ = links.joins(F.SUPPORT)
    got_chains, cycles = scaffoldChains(e1, e2, with_cycles=True)
    assert (got_chains, cycles) == chains(e1.tolist(), e2.tolist())
    # and by content against the oracle's ids: the same sets of members, the same adjacent pairs, as many cycles
    want_chains, want_cycles = chains([j[0] for j in want_joins], [j[1] for j in want_joins])
    as_sets = lambda cs, ks: sorted(sorted(ks[e] for e in ch) for ch in cs)
    assert cycles == want_cycles and as_sets(got_chains, keys) == as_sets(want_chains, okeys)
    assert sorted((keys[a], keys[b]) for ch in got_chains for a, b in zip(ch, ch[1:])) == sorted((okeys[a], okeys[b]) for ch in want_chains for a, b in zip(ch, ch[1:]))
    # one workgroup
    uses = ctx.grid_cap_uses()
    ctx.set_option("test_max_grid", 1)
    try:
        links1, cls1 = LG.link(g, vm, c.pairs, min_len=0, max_span=F.LINK_SPAN + k)
    finally:
        ctx.set_option("test_max_grid", 0)
    assert ctx.grid_cap_uses() > uses and cls1 == want_cls and LG.content(links1, keys) == by_content(want_links, okeys)
    for x in (links, links1, vm, g, m):
        x.close()


@pytest.mark.parametrize("k, variant", CASES)
def test_edge_coverage_and_place(ctx, k, variant):
    c = F.case(k, F.SEEDS[k], variant)
    m, g, vm = build(ctx, c)
    edges, ids, cov = EC.check(g, m, c.counts())
    assert any(classify(s + q) == "self_twin" for s, _, q in edges)
    if k % 2 == 0:
        pal = lambda s, q: any((s + q)[d:d + k] == R.rev_comp((s + q)[d:d + k]) for d in range(len(q) + 1))
        assert any(pal(s, q) and classify(s + q) == "self_twin" for s, _, q in edges)          # the hairpin's centre window
        assert any(s == R.rev_comp(s) for s, _, _ in edges)                                     # the palindromic node as a start
    by_edge = dict(zip(edges, cov))
    for s, e, q in edges:                                                                       # twins read the same numbers
        rp = R.rev_comp(s + q)
        assert by_edge[(rp[:k], rp[len(q):], rp[k:])] == by_edge[(s, e, q)]
    # place: the genome as one record, and cut in two inside the inverted repeat
    nodes, bid = SG.by_id(g)
    at, n = F.where(F.SEEDS[k], k, "inverted")
    for records in ([c.genome], [c.genome[:at + n // 2], c.genome[at + n // 2:]]):
        pst, pwant = J.place(k, *live(nodes, bid), records, id_bound=len(bid))
        if variant == "clean" and len(records) == 1:
            assert tuple(pst[x] for x in F.PLACE_CLASSES) == F.TABLE[(k, variant)]["place"]
            assert pst["both_strands"] > 0 and pst["scattered"] > 0 and pst["forward"] > 0
        p = g.place(vm, records)
        assert p.stats() == pst and placed(p) == pwant
        J.identities(pst=p.stats(), live_edges=len(edges))
        p.close()
    for x in (vm, g, m):
        x.close()


# ---- gap filling through the tandem cycle -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", F.KS)
def test_fill_gaps_round_the_tandem_unit(ctx, k):
    """folded_cases.fill_cases on the device's own ids: the chain (edge into the cycle of U U, edge out of it), whose connecting
    paths run 0, 1, 2, .. times round the unit.  Classes, lengths, spliced members, gaps and stats equal fillgaps_ref; that the
    five cases are filled, shared, ambiguous, none and overflow is asserted on the restatement; then once under one workgroup"""
    c = F.case(k, F.SEEDS[k], "clean")
    m, g, vm = build(ctx, c)
    vm.close()
    edges = FG.by_id(g)
    cases = F.fill_cases(edges, k, F.tandem_unit(c))
    assert len(F.cycle_gadgets(edges, F.tandem_unit(c))) == 2                   # one per strand
    fp = g.idFingerprint()
    for (chains_, gaps, tol, me, mp), want_cls in zip(cases, F.FILL_CLASSES_WANTED):
        want = FR.fill(edges, k, chains_, gaps, tol, me, mp)
        assert tuple(want[2]["classes"][0]) == want_cls
        got = FG.compare(g, edges, chains_, gaps, tol, me, mp)
        if want_cls == ("filled",):
            (e, f), = chains_
            assert len(got[0][0]) == 3 and got[0][0][0] == e and got[0][0][2] == f           # the one edge round to the exit, spliced in
    # both strands' gadgets as two chains in one call
    both = [[e, f] for e, f, _a, _b in F.cycle_gadgets(edges, F.tandem_unit(c))]
    L0 = cases[0][1][0][0]
    assert FG.compare(g, edges, both, [[L0], [L0]], 0, 16, 256)[2]["filled"] == 2
    uses = ctx.grid_cap_uses()
    ctx.set_option("test_max_grid", 1)
    try:
        for chains_, gaps, tol, me, mp in cases:
            FG.compare(g, edges, chains_, gaps, tol, me, mp)
    finally:
        ctx.set_option("test_max_grid", 0)
    assert ctx.grid_cap_uses() > uses and g.idFingerprint() == fp
    g.close(); m.close()
