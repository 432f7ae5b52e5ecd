"""gk_graph_thread_spans / _dev and gk_graph_split_edges_by_spans against tests/spans_ref.py (-m gpu): triples, stats and the
edited graph by id, exact.  The restatement gets the device graph's own nodes and edges by id, the sequences from the contigs of
both strands (which name every live edge by id, so that the copies an edit leaves are told apart).  Seeds are chosen on the CPU;
every case first asserts on the restatement alone that the classes it is about are populated."""
import random
import re
from collections import Counter

import numpy as np
import pytest

from genome_amd import _lib as L
from genome_amd import dna
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.graph import SPAN_STATS, SPLIT_EDGE_STATS, THREAD_STATS, HipSpans, Support, buildGraph, loadGraph
from oracle import pyref as R
from spans_ref import SPLIT_STATS, STATS, split_edges, thread_spans
from thread_cases import build_graph, cut_reads, lengths_for, tiling

pytestmark = pytest.mark.gpu

assert SPAN_STATS == STATS and SPLIT_EDGE_STATS == SPLIT_STATS
GLEN = 2400


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def rand_seq(rnd, n):
    return "".join(rnd.choice("AGCT") for _ in range(n))


def planted(seed, r, loci, glen=GLEN):
    """a random genome in which one stretch of r bases lies at `loci` places between distinct flanks"""
    rnd = random.Random(seed)
    g = list(rand_seq(rnd, glen))
    rep = rand_seq(rnd, r)
    step = glen // (loci + 1)
    for i in range(loci):
        at = step * (i + 1) - r // 2 + rnd.randrange(-40, 40)
        g[at:at + r] = rep
    return "".join(g)


def by_id(g):
    """the device graph by id -> (node k-mers or None, edges (start id, end id, sequence) or None)"""
    k = g.k
    nn, ne = g.idBounds()
    ninfo, einfo = g.nodesById(np.arange(nn, dtype=np.uint32)), g.edgesById(np.arange(ne, dtype=np.uint32))
    nodes = [dna.unpack(int(ninfo["lo"][i]), int(ninfo["hi"][i]), k) if ninfo["alive"][i] else None for i in range(nn)]
    c = g.contigs(min_len=0, line_width=0, strands=2)
    paths = {int(m.group(1)): m.group(2) for m in re.finditer(r">e(\d+) [^\n]*\n([ACGT]+)\n", c.text().decode())}
    c.close()
    edges = []
    for e in range(ne):
        if not einfo["alive"][e]:
            edges.append(None)
            continue
        s, t, p = int(einfo["start"][e]), int(einfo["end"][e]), paths[e]
        assert p[:k] == nodes[s] and p[-k:] == nodes[t] and len(p) == k + int(einfo["len"][e]) and dna.BASES[int(einfo["first"][e])] == p[k]
        edges.append((s, t, p[k:]))
    assert len(paths) == sum(x is not None for x in edges)
    return nodes, edges


def restate(g, reads):
    """the restatement on the device graph as it is now -> ({(e, m, f) by id: count}, stats)"""
    nodes, edges = by_id(g)
    nid = [i for i, x in enumerate(nodes) if x is not None]
    eid = [i for i, x in enumerate(edges) if x is not None]
    nrank = {v: i for i, v in enumerate(nid)}
    spans, st = thread_spans(g.k, [nodes[i] for i in nid], [(nrank[edges[e][0]], nrank[edges[e][1]], edges[e][2]) for e in eid], reads)
    return Counter({(eid[e], eid[m], eid[f]): c for (e, m, f), c in spans.items()}), st


def table(sp):
    e, m, f, c = sp.export()
    out = Counter({(int(a), int(b), int(x)): int(y) for a, b, x, y in zip(e, m, f, c)})
    assert len(out) == len(e) and sp.size() == (len(out), sum(out.values()))
    return out


def thread(g, vm, reads, sp=None):
    sp = HipSpans(g.ctx) if sp is None else sp
    return sp, g.threadSpans(vm, sp, dna.reads_to_bin(reads), len(reads))


def crossing_trips(g, spans):
    """how many 64-lane trips lie between the two crossings of the longest spanned edge"""
    _, edges = by_id(g)
    return max(len(edges[m][2]) for _, m, _ in spans) // 64 if spans else 0


# k + 200 with 255-base reads: a span needs the repeat and a base either side, r + 2 <= 255, which holds up to k = 53.  At k = 35 the
# read has 221 windows and the two crossings are 200 apart, so the first lies at window 1..19 and the second at 201..219: only the
# 19 reads that start 1..19 bases before a locus span it.  The reads at step 3 below give at least six of them per locus.
# At k = 64 (the tagged table) the longest repeat a read can span is 253 = k + 189 bases, by the one read that starts a base before
# it; at this seed the step-3 reads hold that read for both loci (chosen on the CPU, asserted on the restatement below).  k = 31
# is the full one-word key.
LONGEST = {11: 200, 31: 200, 35: 200, 64: 255 - 2 - 64}


@pytest.mark.parametrize("k, extra, loci, err", [(k, x, n, e) for k in (11, 31, 35, 64)
                                                 for x, n, e in [(1, 2, 0.0), (2, 3, 0.0), (70, 2, 0.0), (70, 3, 0.01), (LONGEST[k], 2, 0.0)]])
def test_matches_the_restatement(ctx, k, extra, loci, err):
    r = k + extra
    longest = extra == LONGEST[k]
    assert r + 2 <= 255
    gen = planted(k * 100 + extra, r, loci)
    g = build_graph(ctx, k, tiling(gen, 120, 7))
    vm = g.getGraphMap()
    lens = [255] * 150 if longest else lengths_for(k, 200, extra) + [150] * 100
    reads = cut_reads(extra, gen, lens, err)
    L_ = 255 if longest else 150
    reads += [gen[i:i + L_] for i in range(0, GLEN - L_, 3 if longest else 11)]        # k + 200: every locus is spanned whatever the seed
    reads += [gen[i:i + 60] for i in range(0, GLEN - 60, 37)]           # cut so that some start inside the repeat
    want, st = restate(g, reads)
    assert st["spans"] > 0 and st["open"] > 0 and len(want) >= 2
    assert st["crossings"] == st["spans"] + st["interrupted"] + st["open"]
    if err:
        assert st["interrupted"] > 0
    if extra >= 70:                                                   # the two crossings of a span lie in different lane trips
        assert crossing_trips(g, want) >= extra // 64                  # (1 at 70, 2 at 189, 3 at 200)
    sp, got = thread(g, vm, reads)
    assert got == st
    assert table(sp) == want
    sup = Support(ctx)
    assert g.threadReads(vm, sup, (dna.reads_to_bin(reads), len(reads)))["crossings"] == st["crossings"]
    sup.close(); sp.close(); vm.close(); g.close()


@pytest.fixture(scope="module")
def g35(ctx):
    k = 35
    gen = planted(5, k + 70, 3)
    g = build_graph(ctx, k, tiling(gen, 120, 7))
    reads = cut_reads(2, gen, lengths_for(k, 150, 2) + [150] * 100, 0.0) + [gen[i:i + 150] for i in range(0, GLEN - 150, 23)]
    vm = g.getGraphMap()
    yield k, reads, g, vm
    vm.close(); g.close()


def test_streams_accumulation_and_round_trip(ctx, g35):
    k, reads, g, vm = g35
    want, st = restate(g, reads)
    assert st["spans"] > 0
    sp, got = thread(g, vm, reads)
    assert got == st and table(sp) == want
    # the same stream in chunks of at most 1 KiB of records
    ctx.set_option("test_max_stage", 1024)
    try:
        sp2, got2 = thread(g, vm, reads)
    finally:
        ctx.set_option("test_max_stage", 0)
    assert got2 == st and table(sp2) == want
    # the same reads at the fixed stride of 255-base records, resident on the device
    rec = np.zeros((len(reads), 65), np.uint8)
    for i, r in enumerate(reads):
        b = np.frombuffer(dna.reads_to_bin([r]), np.uint8)
        rec[i, :len(b)] = b
    d = ctx.alloc(rec.size + 64)
    ctx.upload(d, rec)
    sp3 = HipSpans(ctx)
    assert g.threadSpansDev(vm, sp3, d, len(reads), 255) == st and table(sp3) == want
    ctx.free(d)
    # a second call adds up
    _, again = thread(g, vm, reads[:90], sp3)
    w2, st2 = restate(g, reads[:90])
    assert again == st2 and table(sp3) == want + w2
    # export -> add reproduces the table; duplicates in a list add up
    sp4 = HipSpans(ctx)
    e, m, f, c = sp3.export()
    sp4.add(e, m, f, c)
    assert table(sp4) == table(sp3)
    sp4.add(e[:2].repeat(2), m[:2].repeat(2), f[:2].repeat(2), [1, 2, 3, 4])
    t4, t3 = table(sp4), table(sp3)
    k0, k1 = (int(e[0]), int(m[0]), int(f[0])), (int(e[1]), int(m[1]), int(f[1]))
    assert t4[k0] == t3[k0] + 3 and t4[k1] == t3[k1] + 7
    # a count that would pass 2^32 - 1: refused, nothing added
    before = table(sp4)
    with pytest.raises(L.GkError) as ei:
        sp4.add([e[0], 9], [m[0], 9], [f[0], 9], [(1 << 32) - 2, 1])
    assert ei.value.code == L.GK_E_CAPACITY and table(sp4) == before
    for x in (sp, sp2, sp3, sp4):
        x.close()


def test_errors_leave_the_spans_unchanged(ctx, g35):
    k, reads, g, vm = g35
    sp, _ = thread(g, vm, reads[:60])
    before = table(sp)
    binb = dna.reads_to_bin(reads)
    other = HipDNAMap(ctx, 31)
    other.count_reads(binb, len(reads))
    g31 = buildGraph(31, other)
    vm31 = g31.getGraphMap()
    with pytest.raises(L.GkError) as ei:
        g.threadSpans(vm31, sp, binb, len(reads))
    assert ei.value.code == L.GK_E_KLEN and table(sp) == before
    vm31.close(); g31.close(); other.close()
    with pytest.raises(L.GkError) as ei:
        g.threadSpans(vm, sp, binb[:-3], len(reads))
    assert ei.value.code == L.GK_E_FORMAT and table(sp) == before
    assert g.threadSpans(vm, sp, b"", 0) == dict.fromkeys(SPAN_STATS, 0) and table(sp) == before
    st5 = np.zeros(5, np.uint64)
    buf = np.frombuffer(binb, np.uint8)
    lib = L.lib()
    assert lib.gk_graph_thread_spans(g.h, None, sp.h, L.ptr(buf, L.C.c_uint8), buf.size, len(reads), L.ptr(st5, L.C.c_uint64)) == L.GK_E_INVALID
    assert lib.gk_graph_thread_spans(g.h, vm.h, None, L.ptr(buf, L.C.c_uint8), buf.size, len(reads), L.ptr(st5, L.C.c_uint64)) == L.GK_E_INVALID
    assert lib.gk_graph_thread_spans(None, vm.h, sp.h, L.ptr(buf, L.C.c_uint8), buf.size, len(reads), L.ptr(st5, L.C.c_uint64)) == L.GK_E_INVALID
    assert table(sp) == before
    # a device record whose length byte exceeds the declared read length
    rec = np.zeros((len(reads), 26), np.uint8)
    for i, r in enumerate(reads):
        b = np.frombuffer(dna.reads_to_bin([r[:100]]), np.uint8)
        rec[i, :len(b)] = b
    rec[5, 0] = 120
    d = ctx.alloc(rec.size + 64)
    ctx.upload(d, rec)
    with pytest.raises(L.GkError) as ei:
        g.threadSpansDev(vm, sp, d, len(reads), 100)
    assert ei.value.code == L.GK_E_FORMAT and table(sp) == before
    ctx.free(d)
    # a position map taken before an edit: its positions name edges that are gone
    g2 = build_graph(ctx, k, reads)
    vm2 = g2.getGraphMap()
    assert g2.removeEdgesById(np.arange(g2.idBounds()[1], dtype=np.uint32)) > 0
    with pytest.raises(L.GkError) as ei:
        g2.threadSpans(vm2, sp, binb, len(reads))
    assert ei.value.code == L.GK_E_STATE and table(sp) == before
    vm2.close(); g2.close(); sp.close()


# ---- the edit ---------------------------------------------------------------------------------------------------------------

def branching(k, seqs):
    """the k-mers of seqs, on both strands, that have two successors or two predecessors among them (they become the nodes that
    are no dead ends)"""
    km = {x[i:i + k] for s in seqs for x in (s, R.rev_comp(s)) for i in range(len(s) - k + 1)}
    pre, suf = Counter(x[:k - 1] for x in km), Counter(x[1:] for x in km)
    return {x for x in km if pre[x[1:]] >= 2 or suf[x[:k - 1]] >= 2}


def pieces(k, seed, lens, join, rep=1):
    """random strings from the first seed at which the sequences join(*pieces) branch at the two ends of the repeat (piece `rep`) and
    nowhere else (chosen on the CPU)"""
    for s in range(seed, seed + 5000):
        rnd = random.Random(s)
        out = [rand_seq(rnd, n) for n in lens]
        u, v = out[rep][:k], out[rep][-k:]
        if branching(k, join(*out)) == {u, v, R.rev_comp(u), R.rev_comp(v)}:
            return out
    raise AssertionError("no seed")


def graph_of(ctx, k, seqs, L_=150):
    """count, build and simplify the error-free reads that tile `seqs` at step 1 -> (graph, reads)"""
    reads = [s[i:i + L_] for s in seqs for i in range(len(s) - L_ + 1)]
    g = build_graph(ctx, k, reads)
    g.simplifyGraph()
    return g, reads


def live_paths(g):
    nodes, edges = by_id(g)
    return sorted(nodes[x[0]] + x[2] for x in edges if x is not None)


def strands(seqs):
    return sorted(list(seqs) + [R.rev_comp(s) for s in seqs])


def spans_of(g, reads):
    vm = g.getGraphMap()
    sp, st = thread(g, vm, reads)
    vm.close()
    return sp, st


def check_edit(g, sp, cutoff):
    """splitEdgesBySpans against the restatement, by id -> the stats"""
    nodes, edges = by_id(g)
    want_nodes, want_edges, want_st = split_edges(nodes, edges, table(sp), cutoff)
    st = g.splitEdgesBySpans(sp, cutoff)
    assert st == want_st
    assert g.idBounds() == (len(want_nodes), len(want_edges))
    assert by_id(g) == (want_nodes, want_edges)
    n, e, ln = g.counts()
    assert (n, e, ln) == (sum(x is not None for x in want_nodes), sum(x is not None for x in want_edges), sum(len(x[2]) for x in want_edges if x))
    return st


@pytest.mark.parametrize("k", [11, 31, 35, 64])
def test_end_to_end_a_repeat_longer_than_k_becomes_one_contig(ctx, k):
    r = k + 60
    A, Rp, B, C = pieces(k, k, [300, r, 280, 310], lambda A, Rp, B, C: [A + Rp + B + Rp + C])
    gen = A + Rp + B + Rp + C
    g, reads = graph_of(ctx, k, [gen])
    # before: the tangle.  Per strand A into the repeat, the repeat, B from its end back to its start, C out of it
    assert live_paths(g) == strands([A + Rp[:k], Rp, Rp[-k:] + B + Rp[:k], Rp[-k:] + C])
    sp, st = spans_of(g, reads)
    assert st["spans"] > 0 and st["interrupted"] == 0
    est = check_edit(g, sp, 3)
    assert (est["candidates"], est["resolved"], est["new_edges"], est["new_nodes"]) == (2, 2, 2, 4)
    g.simplifyGraph()
    assert live_paths(g) == strands([gen])
    sp.close(); g.close()


def test_end_to_end_two_sequences_come_out_whole(ctx):
    k = 35
    A, Rp, B, C, D = pieces(k, 3, [300, k + 60, 280, 310, 290], lambda A, Rp, B, C, D: [A + Rp + B, C + Rp + D])
    seqs = [A + Rp + B, C + Rp + D]
    g, reads = graph_of(ctx, k, seqs)
    assert len(live_paths(g)) == 10
    sp, _ = spans_of(g, reads)
    # the table of a strand-closed graph is strand-closed: (e, m, f) counts what (twin f, twin m, twin e) counts (the twin of an
    # edge is the edge that spells its reverse complement, as thread_ref.twin_edges pairs them; before the edit no two edges
    # spell the same)
    nodes, edges = by_id(g)
    path = {e: nodes[x[0]] + x[2] for e, x in enumerate(edges) if x is not None}
    by_path = {p: e for e, p in path.items()}
    assert len(by_path) == len(path)
    twin = {e: by_path[R.rev_comp(p)] for e, p in path.items()}
    t = table(sp)
    assert len(t) == 4 and all(t[(twin[f], twin[m], twin[e])] == c for (e, m, f), c in t.items())
    # the new graph and the resolved set are closed under twins, by sequence
    old_edges = g.idBounds()[1]
    est = check_edit(g, sp, 3)
    assert est["resolved"] == 2 and est["new_edges"] == 2
    paths = live_paths(g)
    assert paths == sorted(R.rev_comp(p) for p in paths)
    nodes, edges = by_id(g)
    copies = sorted(nodes[x[0]] + x[2] for x in edges[old_edges:])
    assert copies == strands([Rp]) == sorted(R.rev_comp(p) for p in copies)
    # the edited, not yet simplified graph through a file
    import os
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        g.save(os.path.join(d, "g.graph"))
        g2 = loadGraph(ctx, os.path.join(d, "g.graph"))
        assert g2.counts() == g.counts() and g2.checksum() == g.checksum() and g2.idBounds() == g.idBounds()
        assert by_id(g2) == by_id(g)
        g2.close()
    # a second call with the same, now stale, table: the restatement decides (nothing is a candidate any more)
    assert check_edit(g, sp, 3)["new_edges"] == 0
    g.simplifyGraph()
    assert live_paths(g) == strands(seqs)
    sp.close(); g.close()


def test_reads_shorter_than_the_repeat_leave_it_unsupported(ctx):
    k = 35
    A, Rp, B, C = pieces(k, 8, [200, k + 60, 180, 210], lambda A, Rp, B, C: [A + Rp + B + Rp + C])
    g, _ = graph_of(ctx, k, [A + Rp + B + Rp + C])
    gen = A + Rp + B + Rp + C
    sp, st = spans_of(g, [gen[i:i + 96] for i in range(len(gen) - 96 + 1)])          # a span takes the repeat and a base either side: r + 2 = 97
    assert st["spans"] == 0 and st["open"] > 0
    before = by_id(g)
    est = check_edit(g, sp, 1)
    assert est["candidates"] == 2 and est["unsupported"] == 2 and by_id(g) == before
    sp.close(); g.close()


def test_ambiguous_cutoff_and_unequal_with_added_spans(ctx):
    k = 35
    A, Rp, B, C, D, E = pieces(k, 21, [200, k + 40, 180, 210, 190, 170], lambda A, Rp, B, C, D, E: [A + Rp + B, C + Rp + D, E + Rp + D[:160]])
    # three ways into the repeat, two out of it: unequal
    g, reads = graph_of(ctx, k, [A + Rp + B, C + Rp + D, E + Rp + D[:160]])
    sp, st = spans_of(g, reads)
    assert st["spans"] > 0
    est = check_edit(g, sp, 1)
    assert est["candidates"] == 2 and est["unequal"] == 2 and est["new_edges"] == 0
    sp.close(); g.close()
    # two in, two out: the table of the reads, then with counts of our own
    g, reads = graph_of(ctx, k, [A + Rp + B, C + Rp + D])
    sp, _ = spans_of(g, reads)
    t = table(sp)
    assert len(t) == 4 and min(t.values()) >= 10
    (e0, m0, f0), c0 = sorted(t.items())[0]
    other_f = [f for (e, m, f) in t if m == m0 and f != f0][0]
    # cutoff met exactly: resolved on both strands; one above the smallest count: that pair is missed
    lo = min(t.values())
    nodes, edges = by_id(g)
    assert split_edges(nodes, edges, t, lo)[2]["resolved"] == 2
    assert split_edges(nodes, edges, t, lo + 1)[2]["unsupported"] >= 1
    assert check_edit(g, sp, max(t.values()) + 1)["unsupported"] == 2          # nothing edited
    amb = HipSpans(ctx)
    amb.add(*sp.export())
    amb.add([e0], [m0], [other_f], [c0])                                       # e0 now pairs with both ways out
    nodes, edges = by_id(g)
    assert split_edges(nodes, edges, table(amb), c0)[2]["ambiguous"] == 1
    est = check_edit(g, amb, c0)
    assert est["ambiguous"] == 1
    with pytest.raises(L.GkError) as ei:
        g.splitEdgesBySpans(sp, 0)
    assert ei.value.code == L.GK_E_INVALID
    assert check_edit(g, sp, lo)["new_edges"] + est["new_edges"] == 2
    amb.close(); sp.close(); g.close()
