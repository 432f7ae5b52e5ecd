"""gk_graph_thread_reads / _dev against tests/thread_ref.py (-m gpu): the support by content and all seven stats, exact.

On a fresh graph the restatement runs on the ORACLE's graph of the same reads (content only: no ids, no device); on a graph
after a node split or a merge it gets the device graph's own nodes and edges by id (thread_cases.device_graph).  Every case
first asserts on the restatement alone that the classes it is about are populated."""
import random
from collections import Counter

import numpy as np
import pytest

from genome_amd import _lib as L
from genome_amd import dna
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.graph import THREAD_STATS, Support, buildGraph
from oracle import oracle as O
from oracle import pyref as R
from pairs_ref import gpu_support_by_content, make_pairs, oracle_canonical
from thread_cases import build_graph, cut_reads, genome, lengths_for, restate, tiling
from thread_ref import STATS, thread_reads

pytestmark = pytest.mark.gpu

U32_MAX = (1 << 32) - 1
assert THREAD_STATS == STATS


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def oracle_restate(k, graph_reads, min_count, reads):
    """the restatement on the oracle's graph of graph_reads -> (support by content, stats)"""
    ref = O.PMap(k, 1)
    ref.count_reads(dna.reads_to_bin(graph_reads), len(graph_reads))
    if min_count > 1:
        ref.delete_lt(min_count)
    nodes, oedges = oracle_canonical(O.Graph(ref))
    at = {s: i for i, s in enumerate(nodes)}
    edges = [(at[s], at[t], q) for s, t, q in oedges]
    keys = [(s, dna.BASES.index(q[0])) for s, _, q in oedges]
    sup, st = thread_reads(k, nodes, edges, reads)
    return Counter({(keys[e], keys[f]): c for (e, f), c in sup.items()}), st


def triples(sup):
    e1, e2, cnt = sup.items()
    o = np.lexsort((e2, e1))
    return np.stack([e1[o], e2[o], cnt[o]]).astype(np.uint64)


def snapshot(sup):
    return triples(sup).tolist(), sup.sizes()


def thread(g, vm, reads, sup=None):
    """-> (support, stats) of threading `reads` as a host stream"""
    sup = Support(g.ctx) if sup is None else sup
    return sup, g.threadReads(vm, sup, (dna.reads_to_bin(reads), len(reads)))


def case_reads(k, err, n=300, seed=1):
    return cut_reads(seed, genome(seed, k), lengths_for(k, n, seed), err)


@pytest.mark.parametrize("err", [0.0, 0.01])
@pytest.mark.parametrize("k", [21, 31, 34, 47, 64])
def test_matches_the_restatement(ctx, k, err):
    reads = case_reads(k, err)
    min_count = 2 if err else 1
    want_sup, want = oracle_restate(k, reads, min_count, reads)
    assert want["records"] < len(reads) and want["crossings"] > 0 and want["on_edge"] > 0 and len(want_sup) >= 8
    if err:
        assert want["off_graph"] > 0 and want["broken"] > 0
    assert max(len(r) for r in reads) == 255 and {k + 1, k + 2, k + 63, k + 64, k + 65} <= {len(r) for r in reads}
    g = build_graph(ctx, k, reads, min_count)
    before = g.checksum(), g.idFingerprint()
    vm = g.getGraphMap()
    sup, got = thread(g, vm, reads)
    assert got == want
    assert gpu_support_by_content(g, k, sup) == want_sup
    assert sup.sizes()[1:] == (0, 0)                       # bad pairs and walked orientations do not move
    assert (g.checksum(), g.idFingerprint()) == before
    # twin symmetry on the device: the reverse complements of the reads are the same evidence
    sup2, got2 = thread(g, vm, [R.rev_comp(r) for r in reads])
    assert got2 == want and snapshot(sup2) == snapshot(sup)
    for x in (sup, sup2, vm, g):
        x.close()


@pytest.fixture(scope="module")
def g21(ctx):
    """one graph at k = 21 for the cases that are about the stream, the launch or the support, not about the graph"""
    k = 21
    reads = case_reads(k, 0.0, n=300, seed=2)
    g = build_graph(ctx, k, reads)
    vm = g.getGraphMap()
    yield k, reads, g, vm
    vm.close(); g.close()


@pytest.mark.parametrize("n", [1, 64, 65])
def test_tile_edges(g21, n):
    k, reads, g, vm = g21
    sel = [r for r in reads if len(r) >= k + 40][:n]
    want_sup, want = restate(g, sel)
    assert want["records"] == n and want["on_edge"] > 0
    sup, got = thread(g, vm, sel)
    assert got == want and gpu_support_by_content(g, k, sup) == want_sup
    sup.close()


def test_ragged_host_fixed_stride_and_dev_are_identical(ctx, g21):
    k, reads, g, vm = g21
    sup, st = thread(g, vm, reads)
    assert st["crossings"] > 0
    base = snapshot(sup)
    # the same stream in chunks of at most 1 KiB of records
    ctx.set_option("test_max_stage", 1024)
    try:
        sup2, st2 = thread(g, vm, reads)
    finally:
        ctx.set_option("test_max_stage", 0)
    assert st2 == st and snapshot(sup2) == base
    # the same reads at the fixed stride of 255-base records, resident on the device
    stride = 1 + 64
    rec = np.zeros((len(reads), stride), np.uint8)
    for i, r in enumerate(reads):
        b = np.frombuffer(dna.reads_to_bin([r]), np.uint8)
        rec[i, :len(b)] = b
    d = ctx.alloc(rec.size + 64)
    ctx.upload(d, rec)
    sup3 = Support(ctx)
    st3 = g.threadReadsDev(vm, sup3, d, len(reads), 255)
    assert st3 == st and snapshot(sup3) == base
    ctx.free(d)
    # a record whose length byte exceeds the declared read length: clamped, reported, the support untouched
    stride = 1 + 25
    rec = np.zeros((len(reads), stride), np.uint8)
    for i, r in enumerate(reads):
        b = np.frombuffer(dna.reads_to_bin([r[:100]]), np.uint8)
        rec[i, :len(b)] = b
    rec[5, 0] = 120
    d = ctx.alloc(rec.size + 64)
    ctx.upload(d, rec)
    with pytest.raises(L.GkError) as ei:
        g.threadReadsDev(vm, sup3, d, len(reads), 100)
    assert ei.value.code == L.GK_E_FORMAT and snapshot(sup3) == base
    ctx.free(d)
    for x in (sup, sup2, sup3):
        x.close()


def test_every_record_its_own_chunk(ctx, g21):
    """a staging limit of one byte: every piece is a single record, so both staging areas and the copy stream's event
    alternate on every record"""
    k, reads, g, vm = g21
    sel = reads[::7][:40]
    assert len(sel) == 40 and len({len(r) for r in sel}) >= 5
    want_sup, want = restate(g, sel)
    assert 0 < want["records"] <= 40 and want["crossings"] > 0
    sup, st = thread(g, vm, sel)                                   # unchunked
    assert st == want and gpu_support_by_content(g, k, sup) == want_sup
    ctx.set_option("test_max_stage", 1)
    try:
        sup2, st2 = thread(g, vm, sel)
    finally:
        ctx.set_option("test_max_stage", 0)
    assert st2 == st and snapshot(sup2) == snapshot(sup)
    for x in (sup, sup2):
        x.close()


def test_one_workgroup_and_the_combine_give_the_same(ctx, g21):
    k, reads, g, vm = g21
    sup, st = thread(g, vm, reads)
    base = snapshot(sup)
    uses = ctx.grid_cap_uses()
    ctx.set_option("test_max_grid", 1)
    try:
        sup2, st2 = thread(g, vm, reads)                    # 300 records = 5 tiles on one workgroup
    finally:
        ctx.set_option("test_max_grid", 0)
    assert ctx.grid_cap_uses() > uses
    assert st2 == st and snapshot(sup2) == base
    ctx.set_option("thread_combine", 1)
    try:
        sup3, st3 = thread(g, vm, reads)
    finally:
        ctx.set_option("thread_combine", -1)
    assert st3 == st and snapshot(sup3) == base
    for x in (sup, sup2, sup3):
        x.close()


PAIR_RANGE = (60, 95)                                   # (the walks measure between the mates' first k-mers: make_pairs' 80..100 less k)


def pairs_case(ctx, k=21, seed=1):
    """test_pairs_gpu.py's fixture, on which the walks are known to give support and a split at cutoff 3"""
    reads = make_pairs(seed, k)
    g = build_graph(ctx, k, reads, min_count=2)
    return reads, g


def test_after_a_split_and_after_a_merge(ctx):
    k = 21
    reads, g = pairs_case(ctx)
    vm = g.getGraphMap()
    walked = Support(ctx)
    g.walkPairs(vm, walked, dna.reads_to_bin(reads), len(reads) // 2, *PAIR_RANGE)
    removed, new_nodes = g.splitBySupport(walked, 3)
    assert new_nodes > 0
    vm.close()
    for stage in ("split", "merged"):
        if stage == "merged":
            g.simplifyGraph()
        vm = g.getGraphMap()
        want_sup, want = restate(g, reads)
        # The split visits every node that has in- and out-edges and moves its groups to COPIES: the k-mer of every node a read
        # can cross then has two positions or more, so what was a crossing is `repeated` (and the support may be empty).
        assert want["repeated"] > 0 and want["on_edge"] > 0
        if stage == "merged":
            assert g.counts() != split_counts               # the merge did change the edges the positions name
        split_counts = g.counts()
        sup, got = thread(g, vm, reads)
        assert got == want, stage
        assert gpu_support_by_content(g, k, sup) == want_sup, stage
        sup.close(); vm.close()
    walked.close(); g.close()


def test_accumulation(ctx, g21):
    k, reads, g, vm = g21
    a, b = reads[:140], reads[140:]
    whole, st = thread(g, vm, reads)
    sup, st_a = thread(g, vm, a)
    _, st_b = thread(g, vm, b, sup)
    assert {key: st_a[key] + st_b[key] for key in st} == st
    assert snapshot(sup) == snapshot(whole)
    whole.close(); sup.close()
    # on top of a walked support: the sum of the two, and the walk's counters stay
    preads, pg = pairs_case(ctx)
    pvm = pg.getGraphMap()
    binb = dna.reads_to_bin(preads)
    walked, both = Support(ctx), Support(ctx)
    pg.walkPairs(pvm, walked, binb, len(preads) // 2, *PAIR_RANGE)
    pg.walkPairs(pvm, both, binb, len(preads) // 2, *PAIR_RANGE)
    only, _ = thread(pg, pvm, preads)
    thread(pg, pvm, preads, both)
    w, t, s = (Counter({(int(x), int(y)): int(c) for x, y, c in zip(*q.items())}) for q in (walked, only, both))
    assert w and t and s == w + t
    assert both.sizes()[1:] == walked.sizes()[1:]
    for x in (walked, both, only, pvm, pg):
        x.close()


def test_overflow_leaves_the_support_as_it_was(g21):
    k, reads, g, vm = g21
    sup, _ = thread(g, vm, reads)
    e1, e2, cnt = sup.items()
    i = int(np.argmax(cnt))
    assert cnt[i] >= 2                                      # the reads cross this pair at least twice
    sup.close()
    sup = Support(g.ctx)
    sup.add([e1[i]], [e2[i]], [U32_MAX - 1], bad=5, walked=7)
    before = snapshot(sup)
    with pytest.raises(L.GkError) as ei:
        thread(g, vm, reads, sup)
    assert ei.value.code == L.GK_E_CAPACITY
    assert snapshot(sup) == before
    sup.close()


def test_errors_leave_the_support_unchanged(ctx, g21):
    k, reads, g, vm = g21
    sup, st = thread(g, vm, reads[:50])
    before = snapshot(sup)
    binb = dna.reads_to_bin(reads)
    # a position map of another k
    other = HipDNAMap(ctx, 31)
    other.count_reads(binb, len(reads))
    g31 = buildGraph(31, other)
    vm31 = g31.getGraphMap()
    with pytest.raises(L.GkError) as ei:
        g.threadReads(vm31, sup, (binb, len(reads)))
    assert ei.value.code == L.GK_E_KLEN and snapshot(sup) == before
    vm31.close(); g31.close(); other.close()
    # a stream cut inside a record
    with pytest.raises(L.GkError) as ei:
        g.threadReads(vm, sup, (binb[:-3], len(reads)))
    assert ei.value.code == L.GK_E_FORMAT and snapshot(sup) == before
    # no reads: fine, zero stats
    assert g.threadReads(vm, sup, (b"", 0)) == dict.fromkeys(THREAD_STATS, 0) and snapshot(sup) == before
    # a position map taken before an edit: its positions name edges that are gone
    g2 = build_graph(ctx, k, reads)
    vm2 = g2.getGraphMap()
    _, ne = g2.idBounds()
    assert g2.removeEdgesById(np.arange(ne, dtype=np.uint32)) > 0
    with pytest.raises(L.GkError) as ei:
        g2.threadReads(vm2, sup, (binb, len(reads)))
    assert ei.value.code == L.GK_E_STATE and snapshot(sup) == before
    vm2.close(); g2.close(); sup.close()


@pytest.mark.parametrize("world", [2, 3])
def test_ranks_thread_their_shares_and_reduce(ctx, g21, world):
    from test_pairs_dist_gpu import run_ranks
    k, reads, g, vm = g21
    one, _ = thread(g, vm, reads)
    want = gpu_support_by_content(g, k, one)
    one.close()
    assert len(want) >= 8

    def body(rank, c, hd):
        rg = build_graph(c, k, reads)                       # this rank's replica, on its own context
        rvm = rg.getGraphMap()
        share = reads[len(reads) * rank // world:len(reads) * (rank + 1) // world]
        sup, _ = thread(rg, rvm, share)
        hd.reduce_support(rg, sup)
        out = gpu_support_by_content(rg, k, sup), sup.sizes()[1:]
        sup.close(); rvm.close(); rg.close()
        return out

    for got, counters in run_ranks(world, body):
        assert got == want and counters == (0, 0)


def two_by_two_nodes(g):
    nn, _ = g.idBounds()
    info = g.nodesById(np.arange(nn, dtype=np.uint32))
    return int(np.sum(info["alive"] & (info["in_deg"] >= 2) & (info["out_deg"] >= 2)))


def test_end_to_end_reads_alone_resolve_a_k_long_repeat(ctx):
    k, seed, cutoff = 31, 5, 2
    gen = genome(seed, k, glen=1200, nrep=1)
    rep = next(gen[i:i + k] for i in range(len(gen) - k + 1) if gen.count(gen[i:i + k]) == 2)
    a, b = gen.index(rep), gen.rindex(rep)
    truths = [gen[a - 12:a + k + 12], gen[b - 12:b + k + 12]]      # the two true paths through the repeat
    assert gen[a - 1] != gen[b - 1] and gen[a + k] != gen[b + k]   # distinct flanks: one 2-in / 2-out node (and its twin)
    reads = tiling(gen, 100, 9)

    def paths(g):
        nodes, edges = g.canonical()
        return [s + q for s, _, q in edges]

    def holds(g, t):
        return any(t in p or R.rev_comp(t) in p for p in paths(g))

    outcomes = {}
    for evidence in (True, False):
        g = build_graph(ctx, k, reads)
        assert two_by_two_nodes(g) == 2 and not any(holds(g, t) for t in truths)
        vm, sup = g.getGraphMap(), Support(ctx)
        if evidence:
            st = g.threadReads(vm, sup, (dna.reads_to_bin(reads), len(reads)))
            assert st["crossings"] > 0 and st["broken"] == 0 and st["off_graph"] == 0
        g.splitBySupport(sup, cutoff)
        g.simplifyGraph()
        outcomes[evidence] = (two_by_two_nodes(g), [holds(g, t) for t in truths])
        sup.close(); vm.close(); g.close()
    assert outcomes[True] == (0, [True, True])
    assert outcomes[False] == (0, [False, False])                   # the empty support cuts the connections instead
