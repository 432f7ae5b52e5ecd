"""gk_dist_reduce_links over 2, 3 and 8 loopback ranks (-m gpu).  The link table is a sum over pair orientations and every
orientation is linked on one rank only, so the element-wise sum of the ranks' tables IS the table of one rank linking all the
pairs: each rank's reduced table is compared, by id and exactly, with one pairLinks of ALL pairs on that rank's own replica, and
across ranks by content (an edge is its path).  The odd ranks build their replica from a table of another layout
(test_pairs_dist_gpu.rank_graph), rank world // 2 gets no pairs.  The edited case runs on the graph after reduce_support,
splitBySupport and simplifyGraph — the graph links are taken on, which gk_dist_reduce_support's numbering cannot serve."""
from collections import Counter

import numpy as np
import pytest

from genome_amd import _lib as L
from genome_amd import dna
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.graph import HipLinks, buildGraph
from oracle import pyref as R
from test_pairs_dist_gpu import pair_shares, rank_graph, run_ranks, walk_share
from test_pairs_gpu import make_pairs
from test_pathkey_gpu import paths_by_id
from test_spans_gpu import graph_of, pieces, spans_of

pytestmark = pytest.mark.gpu
RNG = (60, 95)


def records(links):
    """the table as a sorted list of (e, f, count, sum_u)"""
    return sorted(zip(*(a.tolist() for a in links.export())))


def link_share(c, g, vm, binb, share):
    lk = HipLinks(c)
    a, b = share
    cls = g.pairLinks(vm, (dna.bin_pairs(binb, a, b), b - a), lk) if b > a else {"linked": 0}
    return lk, cls


def by_content(recs, paths):
    out = {(paths[e], paths[f]): (c, s) for e, f, c, s in recs}
    assert len(out) == len(recs)
    return out


@pytest.mark.parametrize("edited", [False, True])
@pytest.mark.parametrize("world,k,seed", [(2, 21, 1), (3, 21, 1), (8, 35, 4)])
def test_sum_over_ranks_equals_one_rank(world, k, seed, edited):
    reads = make_pairs(seed, k)
    binb = dna.reads_to_bin(reads)
    nreads, npairs = len(reads), len(reads) // 2
    # (pair_shares leaves rank world // 2 without pairs: with two ranks both get some, so that two ranks contribute)
    shares = pair_shares(npairs, world) if world > 2 else [(0, npairs // 3), (npairs // 3, npairs)]

    def body(rank, c, hd):
        full, g = rank_graph(c, hd, k, binb, nreads, rank, world, False, retain=True, other_layout=rank % 2 == 1)
        res = {}
        if edited:
            vm = g.getGraphMap()
            sup = walk_share(c, g, vm, binb, shares[rank], RNG)
            hd.reduce_support(g, sup)
            res["split"] = g.splitBySupport(sup, 3)
            g.simplifyGraph()
            vm.close()
            try:
                hd.reduce_support(g, sup)
                res["old"] = None
            except L.GkError as e:
                res["old"] = e.code
            sup.close()
        vm = g.getGraphMap()
        whole, _ = link_share(c, g, vm, binb, (0, npairs))       # one pairLinks of every pair on THIS replica: the by-id reference
        res["one"] = records(whole)
        lk, cls = link_share(c, g, vm, binb, shares[rank])
        res["mine"], res["linked"] = records(lk), cls["linked"]
        fp = g.idFingerprint()
        hd.reduce_links(g, lk)
        res["sum"], res["size"] = records(lk), lk.size()
        paths = paths_by_id(g)
        res["content"] = by_content(res["sum"], paths)
        res["renumbered"] = g.idFingerprint() != fp
        whole.close(); lk.close(); vm.close(); g.close(); full.close()
        return res

    out = run_ranks(world, body)
    assert (out[world // 2]["mine"] == []) == (world > 2) and sum(o["linked"] > 0 for o in out) >= 2
    assert sum(c for o in out for _, _, c, _ in o["mine"]) == sum(c for _, _, c, _ in out[0]["one"]) > 0
    for o in out:
        if edited:
            assert o["split"][1] > 0                              # the split made new nodes ...
            assert o["old"] == L.GK_E_STATE                       # ... and the numbering by (start k-mer, first base) refuses the graph
        assert not o["renumbered"]
        assert o["sum"] == o["one"] and o["sum"] != o["mine"]
        assert o["size"] == (len(o["sum"]), sum(r[2] for r in o["sum"]))
        assert o["content"] == out[0]["content"]


@pytest.mark.parametrize("world", [2, 3])
def test_strand_closure_of_the_summed_table(world):
    """On a strand-closed graph (nothing retained, nothing edited: every edge has its reverse-complement twin) count and sum_u of
    (e, f) in the SUMMED table equal those of (twin f, twin e), twins found by path on the host.  The shares are pair_shares':
    at world 2 rank 1 has no pairs and the whole sum is rank 0's."""
    k = 21
    reads = make_pairs(1, k)
    binb = dna.reads_to_bin(reads)
    shares = pair_shares(len(reads) // 2, world)

    def body(rank, c, hd):
        full, g = rank_graph(c, hd, k, binb, len(reads), rank, world, False, retain=False, other_layout=rank % 2 == 1)
        vm = g.getGraphMap()
        lk, _ = link_share(c, g, vm, binb, shares[rank])
        mine = records(lk)
        hd.reduce_links(g, lk)
        res = (mine, records(lk), paths_by_id(g))
        lk.close(); vm.close(); g.close(); full.close()
        return res

    out = run_ranks(world, body)
    assert out[world // 2][0] == []
    for _mine, summed, paths in out:
        by_path = {p: e for e, p in paths.items()}
        twin = {e: by_path[R.rev_comp(p)] for e, p in paths.items()}          # KeyError: the graph is not strand-closed
        table = {(e, f): (c, s) for e, f, c, s in summed}
        assert len(table) >= 6 and any(twin[f] != e for e, f in table)
        assert all(table.get((twin[f], twin[e])) == v for (e, f), v in table.items())


def small_graph(c, k=21, seed=9):
    reads = make_pairs(seed, k, npairs=2000)
    binb = dna.reads_to_bin(reads)
    m = HipDNAMap(c, k)
    m.count_reads(binb, len(reads)); m.deleteAll_lt(2)
    g = buildGraph(k, m)
    m.close()
    return g, binb, len(reads) // 2


@pytest.mark.parametrize("case", ["all_empty", "diverged_replica", "null_table", "late_failure", "overflow", "dead_edge", "duplicate_edge"])
@pytest.mark.parametrize("world", [2, 3])
def test_every_rank_fails_together_and_the_handles_recover(world, case):
    """all_empty: nothing to sum is no error.  The others: every rank raises from the same call, nobody is stuck, every table is
    unchanged, and the same handles then complete a correct reduce."""
    odd = world - 1

    def body(rank, c, hd):
        g, binb, npairs = small_graph(c)
        vm = g.getGraphMap()
        lk, _ = link_share(c, g, vm, binb, (0, 0) if case == "all_empty" else pair_shares(npairs, world)[rank])
        mine = records(lk)
        live = np.flatnonzero(g.edgesById(np.arange(g.idBounds()[1]))["alive"]).tolist()
        target, arg, extra = g, lk, []
        if case == "diverged_replica" and rank == odd:
            target, _, _ = small_graph(c)
            assert target.removeEdgesById([live[0]]) == 1
            extra.append(target)
        elif case == "null_table" and rank == odd:
            arg = None
        elif case == "late_failure" and rank == odd:
            c.set_option("test_dist_fail_reduce", 1)
        elif case == "overflow":
            arg = HipLinks(c)
            if rank < 2:
                arg.add([live[3]], [live[4]], [(1 << 31) + 5], [7])
            arg.add([live[rank]], [live[rank + 1]], [1], [rank])
            extra.append(arg)
        elif case == "dead_edge":
            target, _, _ = small_graph(c)                         # every replica loses the same edge; the odd rank's table names it
            assert target.removeEdgesById([live[0]]) == 1
            arg = HipLinks(c)
            arg.add([live[0] if rank == odd else live[2]], [live[1]], [1], [1])
            extra += [target, arg]
        elif case == "duplicate_edge":
            # A R B R C after splitEdgesBySpans, before simplifyGraph: two live copies of the repeat's edge per strand
            A, Rp, B, Cc = pieces(35, 35, [300, 95, 280, 310], lambda A, Rp, B, Cc: [A + Rp + B + Rp + Cc])
            target, rd = graph_of(c, 35, [A + Rp + B + Rp + Cc])
            sp, _ = spans_of(target, rd)
            assert target.splitEdgesBySpans(sp, 3)["new_edges"] == 2
            sp.close()
            paths = paths_by_id(target)
            copies = [e for e, p in paths.items() if p == Rp]
            plain = [e for e, p in paths.items() if p not in (Rp, R.rev_comp(Rp))]
            assert len(copies) == 2
            arg = HipLinks(c)
            arg.add([plain[0]], [copies[1] if rank == odd else plain[1]], [1], [1])
            extra += [target, arg]
        arg_before = records(arg) if arg is not None else None
        err = None
        try:
            hd.reduce_links(target, arg)
        except L.GkError as e:
            err = (e.code, str(e))
        unchanged = arg is None or records(arg) == arg_before
        still = records(lk) == mine
        hd.reduce_links(g, lk)                                    # the same handles, a correct reduce
        res = (err, unchanged, still, mine, records(lk))
        for x in extra:
            x.close()
        lk.close(); vm.close(); g.close()
        return res

    out = run_ranks(world, body)
    total = Counter()
    for o in out:
        for e, f, c, s in o[3]:
            total[(e, f)] += np.array([c, s], dtype=object)
    want = sorted((e, f, int(v[0]), int(v[1]) % (1 << 64)) for (e, f), v in total.items())
    for rank, (err, unchanged, still, _mine, after) in enumerate(out):
        if case == "all_empty":
            assert err is None and after == []
            continue
        assert err is not None, (case, rank)
        if case == "diverged_replica":
            assert err[0] == L.GK_E_STATE, err
        elif case == "overflow":
            assert err[0] == L.GK_E_CAPACITY, err
        elif case == "null_table":
            assert err[0] == (L.GK_E_INVALID if rank == odd else L.GK_E_COMM), err
        elif case in ("dead_edge", "duplicate_edge"):
            assert err[0] == (L.GK_E_STATE if rank == odd else L.GK_E_COMM), err
        elif case == "late_failure":
            assert ("injected" in err[1]) == (rank == odd), err
        assert unchanged and still, (case, rank)
        assert after == want


def test_world_one_runs_only_the_checks():
    c = Context(0)
    from genome_amd.dist import HipDist, unique_id
    g, binb, npairs = small_graph(c)
    vm = g.getGraphMap()
    hd = HipDist(c, 0, 1, unique_id())
    lk, cls = link_share(c, g, vm, binb, (0, npairs))
    before = records(lk)
    assert cls["linked"] > 0 and before
    hd.reduce_links(g, lk)
    assert records(lk) == before
    # a record that names a dead edge: GK_E_STATE, the table as it was
    e, f = before[0][:2]
    assert g.removeEdgesById([e]) == 1
    with pytest.raises(L.GkError) as err:
        hd.reduce_links(g, lk)
    assert err.value.code == L.GK_E_STATE and records(lk) == before
    with pytest.raises(L.GkError) as err:
        hd.reduce_links(g, None)
    assert err.value.code == L.GK_E_INVALID
    lk.close(); hd.close(); vm.close(); g.close(); c.close()
