"""gk_dist_reduce_spans over 2, 3 and 8 loopback ranks (-m gpu): every rank threads its share of the reads through its own replica
(the odd ranks' built from a table of another capacity, one rank without reads), and each rank's reduced table equals, by id and
exactly, one threadSpans of ALL reads on that rank's replica; across ranks the tables are equal by content (an edge is its path).
The fixture is test_spans_gpu's A R B R C: a repeat longer than k that only reads which span it resolve."""
import random

import pytest

from genome_amd import _lib as L
from genome_amd import dna
from genome_amd.dist_pipeline import simplify_graph
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.freqfilter import PairedEndData
from genome_amd.graph import HipSpans, buildGraph
from test_pairs_dist_gpu import pair_shares, run_ranks
from test_pathkey_gpu import paths_by_id
from oracle import pyref as R
from test_spans_gpu import pieces, table

pytestmark = pytest.mark.gpu
K, L_ = 35, 150


def fixture(k=K):
    A, Rp, B, Cc = pieces(k, k, [300, k + 60, 280, 310], lambda A, Rp, B, Cc: [A + Rp + B + Rp + Cc])
    gen = A + Rp + B + Rp + Cc
    reads = [gen[i:i + L_] for i in range(len(gen) - L_ + 1)]
    random.Random(5).shuffle(reads)                              # (contiguous shares would leave the spanning reads to one rank)
    return gen, reads


def replica(c, reads, rank, k=K):
    m = HipDNAMap(c, k, (1 << 15) * (rank + 1) if rank % 2 else 0)
    m.count_reads(dna.reads_to_bin(reads), len(reads))
    g = buildGraph(k, m)
    m.close()
    g.simplifyGraph()
    return g


def thread_share(c, g, vm, reads, share):
    sp = HipSpans(c)
    a, b = share
    if b > a:
        g.threadSpans(vm, sp, dna.reads_to_bin(reads[a:b]), b - a)
    return sp


@pytest.mark.parametrize("world", [2, 3, 8])
def test_sum_over_ranks_equals_one_rank(world):
    sum_over_ranks(world, K)


def test_sum_over_two_ranks_on_the_tagged_table():
    """k = 64: the spans come from threadSpans on the tagged table, the records travel by path keys whose start k-mer fills both words"""
    sum_over_ranks(2, 64)


def sum_over_ranks(world, k):
    gen, reads = fixture(k)
    # (pair_shares leaves rank world // 2 without reads: with two ranks both get some, so that two ranks contribute)
    shares = pair_shares(len(reads), world) if world > 2 else [(0, len(reads) // 3), (len(reads) // 3, len(reads))]

    def body(rank, c, hd):
        g = replica(c, reads, rank, k)
        vm = g.getGraphMap()
        whole = thread_share(c, g, vm, reads, (0, len(reads)))
        sp = thread_share(c, g, vm, reads, shares[rank])
        res = {"one": table(whole), "mine": table(sp)}
        hd.reduce_spans(g, sp)
        res["sum"] = table(sp)
        paths = paths_by_id(g)
        res["content"] = {(paths[e], paths[m], paths[f]): n for (e, m, f), n in res["sum"].items()}
        # the summed table resolves the repeat: one contig per strand
        st = g.splitEdgesBySpans(sp, 3)
        g.simplifyGraph()
        res["resolved"], res["paths"] = st["resolved"], sorted(paths_by_id(g).values())
        whole.close(); sp.close(); vm.close(); g.close()
        return res

    out = run_ranks(world, body, timeout=120)
    assert (out[world // 2]["mine"] == {}) == (world > 2) and sum(bool(o["mine"]) for o in out) >= 2
    assert sum(sum(o["mine"].values()) for o in out) == sum(out[0]["one"].values()) > 0
    for o in out:
        assert o["sum"] == o["one"] and o["sum"] != o["mine"]
        assert o["content"] == out[0]["content"]
        assert o["resolved"] == 2 and len(o["paths"]) == 2 and gen in o["paths"]


@pytest.mark.parametrize("case", ["late_failure", "overflow"])
def test_every_rank_fails_together_and_the_handles_recover(case):
    world, odd = 2, 1
    _, reads = fixture()

    def body(rank, c, hd):
        g = replica(c, reads, 0)
        vm = g.getGraphMap()
        sp = thread_share(c, g, vm, reads, (0, len(reads)))       # (both ranks all reads: the same triples on both)
        mine = table(sp)
        arg = sp
        if case == "late_failure" and rank == odd:
            c.set_option("test_dist_fail_reduce", 1)
        elif case == "overflow":
            paths = paths_by_id(g)                               # the same triple by CONTENT on both ranks: their ids differ
            e, m, f = min(mine, key=lambda t: tuple(paths[x] for x in t))
            arg = HipSpans(c)
            arg.add([e], [m], [f], [(1 << 31) + 5])
        before = table(arg)
        err = None
        try:
            hd.reduce_spans(g, arg)
        except L.GkError as x:
            err = (x.code, str(x))
        unchanged = table(arg) == before and table(sp) == mine
        hd.reduce_spans(g, sp)
        res = (err, unchanged, mine, table(sp))
        if arg is not sp:
            arg.close()
        sp.close(); vm.close(); g.close()
        return res

    out = run_ranks(world, body, timeout=120)
    for rank, (err, unchanged, _mine, after) in enumerate(out):
        assert err is not None and unchanged
        if case == "overflow":
            assert err[0] == L.GK_E_CAPACITY, err
        else:
            assert ("injected" in err[1]) == (rank == odd), err
        assert after == {key: 2 * n for key, n in _mine.items()}      # both ranks held the same triples, each under its own ids


@pytest.mark.parametrize("world", [2, 3])
def test_a_repeat_longer_than_k_through_the_pipeline(world, tmp_path):
    """A R B R C through dist_pipeline.simplify_graph(resolve_repeats=...): every rank loads the tangle, threads its share of the
    reads, the spans are summed, and every rank ends with one contig per strand."""
    gen, reads = fixture()
    reads = reads[:len(reads) // 2 * 2]
    data = PairedEndData(len(reads) // 2, dna.reads_to_bin(reads))
    path = str(tmp_path / "tangle.gkg")
    c = Context(0)
    g = replica(c, reads, 0)
    before = sorted(paths_by_id(g).values())
    g.save(path)
    g.close(); c.close()
    assert len(before) == 8

    def body(rank, c, hd):
        g, stats = simplify_graph(hd, path, data, 3, walk=False, resolve_repeats=(3, 2))
        res = (sorted(paths_by_id(g).values()), stats["resolve_repeats"], stats["walk_pairs"])
        g.close()
        return res

    for paths, rounds, walk in run_ranks(world, body, timeout=120):
        assert paths == sorted([gen, R.rev_comp(gen)]) and walk is None
        assert rounds[0]["split_edges"]["resolved"] == 2 and rounds[0]["thread_spans"]["spans"] > 0 and rounds == run_rounds(rounds)


def run_rounds(rounds):
    """the rounds as they must be: the first resolves, a second (if any) finds nothing left"""
    assert len(rounds) in (1, 2) and (len(rounds) == 1 or rounds[1]["split_edges"]["resolved"] == 0)
    return rounds
