"""gk_graph_pair_links, the link table and gk_links_joins on the device (-m gpu).  classes8, the exported (e, f, count, sum_u) and the
joins must equal, exactly, what tests/links_ref.py (strings only; held to hand-computed answers by tests/test_links_cpu.py) gives
on the ORACLE's graph of the same reads, compared by content: an edge is its (start k-mer, first base).  Fixtures:
insert_cases.small_pairs, a 2400-base genome with three planted repeats, mates of k + 9 bases, at most 800 pairs with inserts
80..100.  Every case first asserts, on the restatement alone, that the classes it is about are populated."""
import ctypes as C

import numpy as np
import pytest

from genome_amd import _lib as L
from genome_amd import dna
from genome_amd.dnamap import Context, HipDNAMap, HipValueMap
from genome_amd.freqfilter import PairedEndData
from genome_amd.graph import JOIN_STATS, LINK_CLASSES, HipLinks, Support, buildGraph, scaffoldChains
from insert_cases import small_pairs
from links_cases import by_content, oracle_graph, restate, settings
from links_ref import CLASSES, chains, index_graph, joins, pair_links
from pairs_ref import make_pairs
from thread_cases import device_graph as graph_by_id
from thread_ref import twin_edges

pytestmark = pytest.mark.gpu
U32_MAX = (1 << 32) - 1
assert LINK_CLASSES == CLASSES

# what the restatement gives with the settings S (links_cases.settings): linked, distinct links, supported, joins, forking edges
TABLE = {(21, 0.0): (466, 64, 54, 44, 4), (21, 0.01): (412, 50, 42, 30, 4), (31, 0.0): (296, 36, 34, 34, 0), (64, 0.0): (10, 8, 0, 0, 0)}


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def device_graph(ctx, k, reads, min_count=1):
    m = HipDNAMap(ctx, k)
    m.count_reads(dna.reads_to_bin(reads), len(reads))
    if min_count > 1:
        m.deleteAll_lt(min_count)
    g = buildGraph(k, m)
    m.close()
    return g, g.getGraphMap()


def edge_keys(g):
    """edge id -> (start k-mer, first base code), for every live id"""
    ids = np.arange(g.idBounds()[1], dtype=np.uint32)
    info = g.edgesById(ids)
    nid = np.arange(g.idBounds()[0], dtype=np.uint32)
    ninfo = g.nodesById(nid)
    kmer = lambda n: dna.unpack(int(ninfo["lo"][n]), int(ninfo["hi"][n]), g.k)
    return {int(e): (kmer(int(info["start"][e])), int(info["first"][e])) for e in ids if info["alive"][e]}


def records(links):
    """the table as a sorted list of (e, f, count, sum_u)"""
    return sorted(zip(*(a.tolist() for a in links.export())))


def content(links, keys):
    recs = records(links)
    out = {(keys[e], keys[f]): (c, s) for e, f, c, s in recs}
    assert len(out) == len(recs)
    return out


def content_joins(links, keys, support):
    (e1, e2, cnt, su), st = links.joins(support)
    assert e1.dtype == np.uint32 and su.dtype == np.uint64
    assert all(a < b for a, b in zip(e1.tolist(), e1.tolist()[1:]))          # strictly ascending e1
    return sorted((keys[e], keys[f], c, s) for e, f, c, s in zip(e1.tolist(), e2.tolist(), cnt.tolist(), su.tolist())), st


def link(g, vm, reads, npairs=None, links=None, min_len=0, max_span=4095, **kw):
    links = HipLinks(g.ctx) if links is None else links
    npairs = len(reads) // 2 if npairs is None else npairs
    return links, g.pairLinks(vm, (dna.reads_to_bin(reads), npairs), links, min_len=min_len, max_span=max_span, **kw)


# ---- key widths --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("err", [0.0, 0.01])
@pytest.mark.parametrize("k", [21, 31, 34, 47, 64])
def test_every_key_width(ctx, k, err):
    """One word (21, 31), four bits of the high word (34), two words (47), the tagged table (64), error-free and with 1 %
    substitutions under the count filter at 2, with the settings S.  A second call with max_span = 40 + k fills too_far."""
    reads = small_pairs(100 + k, k, err=err, npairs=800 if err else 400)
    min_count = 2 if err else 1
    npairs = len(reads) // 2
    S = settings(k)
    want_links, want_cls, want_joins, want_st = restate(k, reads, reads, npairs, S["min_len"], S["max_span"], S["support"], min_count)
    assert want_cls["at_node"] > 0 and want_cls["same_edge"] > 0 and want_cls["short_edge"] > 0 and want_cls["linked"] > 0
    if err:
        assert want_cls["unplaced"] > 50
    if (k, err) in TABLE:
        assert (want_cls["linked"], want_st["links"], want_st["supported"], want_st["joins"], want_st["forks"]) == TABLE[(k, err)]
    g, vm = device_graph(ctx, k, reads, min_count)
    keys = edge_keys(g)
    before = g.idFingerprint(), vm.size()
    links, cls = link(g, vm, reads, min_len=S["min_len"], max_span=S["max_span"])
    assert cls == want_cls and cls["orientations"] == sum(cls[c] for c in CLASSES[1:])
    assert content(links, keys) == want_links
    assert links.size() == (len(want_links), want_cls["linked"])
    got_joins, st = content_joins(links, keys, S["support"])
    assert got_joins == want_joins and st == want_st
    assert (g.idFingerprint(), vm.size()) == before
    # a prefix through take_first, into a fresh table
    third = HipLinks(ctx)
    cls3 = g.pairLinks(vm, PairedEndData(npairs, dna.reads_to_bin(reads)), third, min_len=S["min_len"], max_span=S["max_span"], take_first=npairs // 3)
    w3 = restate(k, reads, reads, npairs // 3, S["min_len"], S["max_span"], S["support"], min_count)
    assert cls3 == w3[1] and content(third, keys) == w3[0]
    # too_far
    far_links, far_cls, _, _ = restate(k, reads, reads, npairs, S["min_len"], 40 + k, S["support"], min_count)
    assert far_cls["too_far"] > 0
    far, cls_far = link(g, vm, reads, min_len=S["min_len"], max_span=40 + k)
    assert cls_far == far_cls and content(far, keys) == far_links
    for x in (links, third, far, vm, g):
        x.close()


def test_a_supported_link_that_is_no_join_and_the_chains(ctx):
    """k = 21 is the case where a link is supported and is not a join (forks); the chains of its joins, by content, are the
    restatement's"""
    k = 21
    reads = small_pairs(100 + k, k)
    S = settings(k)
    index, lens, okeys, _ = oracle_graph(k, reads)
    olinks, _ = pair_links(k, index, lens, reads, len(reads) // 2, S["min_len"], S["max_span"])
    ojoins, ost = joins(olinks, S["support"])
    assert ost["supported"] > ost["joins"] > 0 and ost["forks"] > 0
    ochains, ocycles = chains([j[0] for j in ojoins], [j[1] for j in ojoins])
    assert any(len(c) >= 3 for c in ochains)
    g, vm = device_graph(ctx, k, reads)
    keys = edge_keys(g)
    links, _ = link(g, vm, reads, min_len=S["min_len"], max_span=S["max_span"])
    (e1, e2, _, _), st = links.joins(S["support"])
    got, cycles = scaffoldChains(e1, e2, with_cycles=True)
    assert sorted([keys[e] for e in c] for c in got) == sorted([okeys[e] for e in c] for c in ochains) and cycles == ocycles
    for x in (links, vm, g):
        x.close()


def test_no_supported_link(ctx):
    """k = 64, error-free: links, none of them seen three times: joins returns n = 0 and GK_OK"""
    k = 64
    reads = small_pairs(100 + k, k)
    S = settings(k)
    _, cls, want_joins, st = restate(k, reads, reads, len(reads) // 2, S["min_len"], S["max_span"], S["support"])
    assert st["links"] > 0 and st["supported"] == 0 and want_joins == []
    g, vm = device_graph(ctx, k, reads)
    links, _ = link(g, vm, reads, min_len=S["min_len"], max_span=S["max_span"])
    (e1, e2, cnt, su), got = links.joins(S["support"])
    assert len(e1) == len(e2) == len(cnt) == len(su) == 0 and got == st
    n, stats = C.c_uint64(7), np.zeros(5, np.uint64)
    assert L.lib().gk_links_joins(links.h, 3, None, None, None, None, 0, C.byref(n), L.ptr(stats, C.c_uint64)) == L.GK_OK and n.value == 0
    empty = HipLinks(ctx)
    assert empty.joins(1)[1] == dict.fromkeys(JOIN_STATS, 0) and empty.size() == (0, 0) and records(empty) == []
    for x in (links, empty, vm, g):
        x.close()


# ---- node copies: repetitive -----------------------------------------------------------------------------------------------------

def test_repetitive_after_a_split(ctx):
    """after gk_graph_split_by_support the copies of a node share a k-mer: its getAll holds two positions or more"""
    k = 21
    reads = make_pairs(1, k)
    g, vm = device_graph(ctx, k, reads, 2)
    walked = Support(ctx)
    g.walkPairs(vm, walked, dna.reads_to_bin(reads), len(reads) // 2, 60, 95)
    _, new_nodes = g.splitBySupport(walked, 3)
    assert new_nodes > 0
    vm.close(); walked.close()
    vm = g.getGraphMap()
    nodes, edges, okeys = graph_by_id(g)
    index, lens = index_graph(k, [(nodes[s], q) for s, _, q in edges], nodes=nodes)
    sel = reads[:1600]
    want_links, want_cls = pair_links(k, index, lens, sel, 800, 2 * k, 100 + k)
    assert want_cls["repetitive"] > 0 and want_cls["linked"] > 0
    links, cls = link(g, vm, sel, min_len=2 * k, max_span=100 + k)
    assert cls == want_cls and content(links, edge_keys(g)) == by_content(want_links, okeys)
    for x in (links, vm, g):
        x.close()


# ---- one graph at k = 31 for the cases that are about the table, the stream or the launch ----------------------------------------

@pytest.fixture(scope="module")
def k31(ctx):
    k = 31
    reads = small_pairs(131, k)
    g, vm = device_graph(ctx, k, reads)
    S = settings(k)
    yield k, reads, g, vm, dict(min_len=S["min_len"], max_span=S["max_span"])
    vm.close(); g.close()


def test_growth_from_70000_links(ctx, k31):
    """70 000 distinct synthetic links first: the table has grown well past its first size when the pairs' links merge into it"""
    k, reads, g, vm, S = k31
    n = 70000
    i = np.arange(n, dtype=np.uint64)
    e1, e2 = (i // 300 + 5000).astype(np.uint32), (i % 300 + 9000).astype(np.uint32)
    cnt, su = (i % 7 + 1).astype(np.uint32), i * 3 + 11
    links = HipLinks(ctx)
    links.add(e1[:100], e2[:100], cnt[:100], su[:100])
    links.add(e1[100:], e2[100:], cnt[100:], su[100:])
    assert links.size() == (n, int(cnt.sum()))
    alone, cls = link(g, vm, reads, **S)
    assert cls["linked"] > 100
    link(g, vm, reads, links=links, **S)
    want = sorted(list(zip(e1.tolist(), e2.tolist(), cnt.tolist(), su.tolist())) + records(alone))
    assert records(links) == want
    # duplicates in a list add up, and add onto what is there
    links.add([5000, 5000], [9000, 9000], [2, 3], [10, 20])
    assert [r for r in records(links) if r[:2] == (5000, 9000)] == [(5000, 9000, int(cnt[0]) + 5, int(su[0]) + 30)]
    # export, then add into an empty table, reproduces the table
    copy = HipLinks(ctx)
    copy.add(*links.export())
    assert records(copy) == records(links)
    for x in (links, alone, copy):
        x.close()


@pytest.mark.parametrize("cap", [1, 3])
def test_grid_cap(k31, cap):
    """800 orientations on 1 and on 3 workgroups of 256 lanes: every lane takes several trips, the last one partly past the end;
    the joins' kernels under the same cap"""
    k, reads, g, vm, S = k31
    assert len(reads) > 3 * 256
    ctx = g.ctx
    free, cls_free = link(g, vm, reads, **S)
    joins_free = free.joins(3)
    assert cls_free["linked"] > 100 and len(joins_free[0][0]) > 10
    ctx.set_option("test_max_grid", cap)
    try:
        uses = ctx.grid_cap_uses()
        capped, cls = link(g, vm, reads, **S)
        joins_capped = capped.joins(3)
        assert ctx.grid_cap_uses() > uses
    finally:
        ctx.set_option("test_max_grid", 0)
    assert cls == cls_free and records(capped) == records(free)
    assert [a.tolist() for a in joins_capped[0]] == [a.tolist() for a in joins_free[0]] and joins_capped[1] == joins_free[1]
    free.close(); capped.close()


def test_accumulation_and_stream_shapes(ctx, k31):
    k, reads, g, vm, S = k31
    npairs = len(reads) // 2
    whole, cls = link(g, vm, reads, **S)
    assert cls["linked"] > 100
    # two calls over two halves equal one call
    half = 2 * (npairs // 2)
    links, a = link(g, vm, reads[:half], **S)
    _, b = link(g, vm, reads[half:], links=links, **S)
    assert {c: a[c] + b[c] for c in CLASSES} == cls and records(links) == records(whole)
    links.close()
    # a ragged stream (cut on the host) gives what the fixed stride (cut on the device) gives
    assert {len(r) for r in reads} == {k + 9}
    ragged = [r[:len(r) - (i % 4) * 3] if i % 3 else r for i, r in enumerate(reads)]
    assert {len(r) for r in ragged} == {k, k + 3, k + 6, k + 9}
    links, got = link(g, vm, ragged, **S)
    assert got == cls and records(links) == records(whole)
    links.close()
    # mates shorter than k drop their pair
    short = list(ragged)
    for i in (0, 7, 200, len(short) - 1):
        short[i] = short[i][:k - 1]
    index, lens, okeys, _ = oracle_graph(k, reads)
    want_links, want_cls = pair_links(k, index, lens, short, npairs, S["min_len"], S["max_span"])
    assert want_cls["orientations"] == 2 * (npairs - 4)
    links, got = link(g, vm, short, **S)
    assert got == want_cls and content(links, edge_keys(g)) == by_content(want_links, okeys)
    links.close()
    # a prefix by npairs
    want_links, want_cls = pair_links(k, index, lens, reads, 100, S["min_len"], S["max_span"])
    for stream in (reads, ragged):
        links, got = link(g, vm, stream, npairs=100, **S)
        assert got == want_cls and content(links, edge_keys(g)) == by_content(want_links, okeys)
        links.close()
    # an empty stream
    before = records(whole)
    assert g.pairLinks(vm, (b"", 0), whole) == dict.fromkeys(CLASSES, 0) and records(whole) == before
    whole.close()


def raw_pair_links(g, vm, links, binb, npairs, S):
    """the C call itself -> (return code, classes8), which starts as a pattern"""
    buf = np.frombuffer(binb, np.uint8)
    cls = np.full(8, 0xabcdef, np.uint64)
    rc = L.lib().gk_graph_pair_links(g.h, vm.h, links.h, L.ptr(buf, C.c_uint8), buf.size, npairs, S["min_len"], S["max_span"], L.ptr(cls, C.c_uint64))
    return rc, cls.tolist()


def test_errors_leave_the_handle_unchanged(ctx, k31):
    k, reads, g, vm, S = k31
    links, cls = link(g, vm, reads[:400], **S)
    before = records(links)
    assert cls["linked"] > 20 and before
    binb = dna.reads_to_bin(reads)
    # a stream cut inside a pair: 100 pairs and one record, in either cut
    ragged = [r[:len(r) - (i % 4) * 3] if i % 3 else r for i, r in enumerate(reads)]
    for stream in (reads, ragged):
        cut = dna.reads_to_bin(stream[:201])
        assert raw_pair_links(g, vm, links, cut, 101, S) == (L.GK_E_FORMAT, [0] * 8) and records(links) == before
        with pytest.raises(L.GkError) as e:
            g.pairLinks(vm, (cut, 101), links, **S)
        assert e.value.code == L.GK_E_FORMAT
    # a position map of another k
    other = HipValueMap(ctx, 21, 64)
    assert raw_pair_links(g, other, links, binb, 10, S) == (L.GK_E_KLEN, [0] * 8) and records(links) == before
    other.close()
    # a position map taken before an edit: its positions name edges that are gone
    g2, vm2 = device_graph(ctx, k, reads)
    assert g2.removeEdgesById(np.arange(g2.idBounds()[1], dtype=np.uint32)) > 0
    assert raw_pair_links(g2, vm2, links, binb, len(reads) // 2, S) == (L.GK_E_STATE, [0] * 8) and records(links) == before
    vm2.close(); g2.close()
    # another context
    c2 = Context(0)
    foreign = HipLinks(c2)
    assert raw_pair_links(g, vm, foreign, binb, 10, S)[0] == L.GK_E_INVALID
    foreign.close(); c2.close()
    assert records(links) == before
    links.close()


def test_counter_limits(ctx, k31):
    k, reads, g, vm, S = k31
    alone, cls = link(g, vm, reads, **S)
    e, f, c, s = max(records(alone), key=lambda r: r[2])
    assert c >= 2
    links = HipLinks(ctx)
    links.add([e, 7], [f, 8], [U32_MAX - c, U32_MAX - 1], [5, 6])
    links.add([7], [8], [1], [1])                              # up to 2^32 - 1 succeeds
    link(g, vm, reads, links=links, **S)                       # and so do the pairs that fill (e, f) to the brim
    full = records(links)
    assert (e, f, U32_MAX, s + 5) in full and (7, 8, U32_MAX, 7) in full and len(full) == len(records(alone)) + 1
    for args in (([7], [8], [1], [0]), ([9, e, 9], [9, f, 9], [1, 1, 1], [0, 0, 0]), ([3, 3], [4, 4], [U32_MAX, 1], [0, 0])):
        with pytest.raises(L.GkError) as ei:
            links.add(*args)
        assert ei.value.code == L.GK_E_CAPACITY and records(links) == full
    with pytest.raises(L.GkError) as ei:
        link(g, vm, reads, links=links, **S)
    assert ei.value.code == L.GK_E_CAPACITY and records(links) == full
    links.close(); alone.close()


def test_strand_closure(ctx, k31):
    """on an unedited graph count and sum_u of (e, f) equal those of (twin f, twin e); twins found by content on the host"""
    k, reads, g, vm, S = k31
    nodes, edges, _ = graph_by_id(g)
    live = sorted(edge_keys(g))                                # graph_by_id's indices are ranks among the live ids
    twin_rank = twin_edges(k, nodes, edges)
    twin = {live[a]: live[b] for a, b in twin_rank.items()}
    links, cls = link(g, vm, reads, **S)
    table = {(e, f): (c, s) for e, f, c, s in records(links)}
    assert len(table) > 20 and any(twin[f] != e for e, f in table)
    assert all(table.get((twin[f], twin[e])) == v for (e, f), v in table.items())
    links.close()


def test_joins_order_and_capacity(ctx, k31):
    k, reads, g, vm, S = k31
    links, _ = link(g, vm, reads, **S)
    (e1, e2, cnt, su), st = links.joins(3)
    n = len(e1)
    assert n == st["joins"] > 10 and all(a < b for a, b in zip(e1.tolist(), e1.tolist()[1:]))
    table = {(e, f): (c, s) for e, f, c, s in records(links)}
    assert all(table[(a, b)] == (c, s) and c >= 3 for a, b, c, s in zip(e1.tolist(), e2.tolist(), cnt.tolist(), su.tolist()))
    got, stats = C.c_uint64(), np.zeros(5, np.uint64)
    out = [np.full(n, 77, np.uint32) for _ in range(3)] + [np.full(n, 77, np.uint64)]
    rc = L.lib().gk_links_joins(links.h, 3, L.ptr(out[0], C.c_uint32), L.ptr(out[1], C.c_uint32), L.ptr(out[2], C.c_uint32), L.ptr(out[3], C.c_uint64), n - 1,
                                C.byref(got), L.ptr(stats, C.c_uint64))
    assert rc == L.GK_E_CAPACITY and got.value == n and dict(zip(JOIN_STATS, stats.tolist())) == st
    assert all((a == 77).all() for a in out)                   # nothing copied
    with pytest.raises(L.GkError) as ei:
        links.joins(3, cap=n - 1)
    assert ei.value.code == L.GK_E_CAPACITY
    assert [a.tolist() for a in links.joins(3, cap=n + 5)[0]] == [e1.tolist(), e2.tolist(), cnt.tolist(), su.tolist()]
    # a higher bar: fewer supported links, joins still a function of the supported ones
    hi = max(cnt.tolist())
    (h1, _, hc, _), hst = links.joins(hi)
    assert 0 < hst["supported"] < st["supported"] and all(c >= hi for c in hc.tolist()) and hst["links"] == st["links"]
    links.close()
