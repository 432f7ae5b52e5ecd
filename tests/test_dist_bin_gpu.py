"""A collective count of host `.bin` streams over N ranks (gk_dist_count_reads, -m gpu) and the N-rank GraphBuilder +
GraphSimplifier pairs pipeline built on it (genome_amd.dist_pipeline, graph_builder --world).

The streams are RAGGED, as Convert2bin writes them: every mate is cut at a random position (lengths 0..150, some up to 255,
some below k).  Ranks are the threads of this process over the test library's loopback transport for world > 1, and RCCL for
world 1.  The union of the ranks' partitions must be the one-rank table of the whole stream (gk_map_count_reads), itself the
oracle's; the pipeline's numbers and final graph must be the one-rank flow's."""
import ctypes as C
import json
import os
import random
import subprocess

import numpy as np
import pytest

from genome_amd import _lib as L
from genome_amd import dna
from genome_amd.dist import DistDNAMap, HipDist, unique_id
from genome_amd.dist_pipeline import build_graph
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.freqfilter import PairedEndData
from genome_amd.graph import Support, buildGraph
from oracle import oracle as O
from test_pairs_dist_gpu import run_ranks
from test_pairs_gpu import gpu_canonical, make_pairs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "genome_amd", "host", "graph_builder")


def ragged_reads(seed, n, glen=6000):
    """n reads of a random genome (both strands), each cut at a random position: mostly 0..150 bases, some up to 255"""
    rnd = random.Random(seed)
    g = "".join(rnd.choice("AGCT") for _ in range(glen))
    reads = []
    for _ in range(n):
        ln = rnd.randint(151, 255) if rnd.random() < 0.08 else rnd.randint(0, 150)
        s = rnd.randrange(0, glen - ln)
        r = g[s:s + ln]
        reads.append(dna.rev_complement(r) if rnd.random() < 0.5 else r)
    return reads


def record_offsets(binb):
    off, pos = [0], 0
    while pos < len(binb):
        pos += 1 + (binb[pos] + 3) // 4
        off.append(pos)
    return off


def read_slices(binb, world, shares=None):
    """the stream cut into `world` contiguous slices of whole records -> [(bytes, nreads)]"""
    off = record_offsets(binb)
    n = len(off) - 1
    shares = shares or [(n * r // world, n * (r + 1) // world) for r in range(world)]
    return [(binb[off[a]:off[b]], b - a) for a, b in shares]


def one_rank_table(binb, nreads, k):
    c = Context(0)
    m = HipDNAMap(c, k, 1 << 10)
    occ = m.count_reads(binb, nreads)
    items = m.sorted_items()
    m.close(); c.close()
    ref = O.PMap(k, 1)
    assert ref.count_reads(binb, nreads) == occ
    for a, b in zip(items, ref.export_sorted()):
        assert np.array_equal(a, b), "the one-rank count is not the oracle's"
    return items, occ


def count_body(slices, k, options=None):
    """per rank: count its slice into a fresh partition -> (sorted items, sent, owned, foreign keys)"""
    options = options or {}

    def body(rank, c, hd):
        for name, v in options.get(rank, {}).items():
            c.set_option(name, v)
        pm = DistDNAMap(hd, k, 1 << 10)
        binb, n = slices[rank]
        sent, owned = pm.count_reads(binb, n)
        foreign = count_foreign(pm.local, hd.world, rank)
        items = pm.local.sorted_items()
        pm.close()
        return items, sent, owned, foreign
    return body


def count_foreign(m, world, rank):
    n = C.c_uint64()
    L.check(L.lib().gk_map_count_foreign(m.h, world, rank, C.byref(n)), m.ctx.h)
    return n.value


def run_world(world, body):
    """world 1 over RCCL (the product transport), world > 1 over the loopback transport"""
    if world > 1:
        return run_ranks(world, body)
    c = Context(0)
    hd = HipDist(c, 0, 1, unique_id())
    try:
        return [body(0, c, hd)]
    finally:
        hd.close(); c.close()


def union(out):
    lo = np.concatenate([o[0][0] for o in out]); hi = np.concatenate([o[0][1] for o in out]); cnt = np.concatenate([o[0][2] for o in out])
    order = np.lexsort((lo, hi))
    return lo[order], hi[order], cnt[order]


def check_same_table(out, want, occ):
    got = union(out)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    assert sum(o[1] for o in out) == occ and sum(o[2] for o in out) == occ
    assert all(o[3] == 0 for o in out), [o[3] for o in out]


# ---- the count ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("world,k", [(1, 21), (2, 31), (3, 35), (2, 63), (3, 21)])
def test_ragged_stream_over_ranks_is_the_one_rank_table(world, k):
    reads = ragged_reads(world * 100 + k, 3000)
    assert any(len(r) < k for r in reads) and any(len(r) > 150 for r in reads) and any(len(r) == 0 for r in reads)
    binb = dna.reads_to_bin(reads)
    want, occ = one_rank_table(binb, len(reads), k)
    out = run_world(world, count_body(read_slices(binb, world), k))
    check_same_table(out, want, occ)


@pytest.mark.parametrize("case", ["all_on_rank0", "one_vs_many_chunks"])
def test_uneven_shares(case):
    world, k = 3, 31
    reads = ragged_reads(11, 2500)
    binb = dna.reads_to_bin(reads)
    want, occ = one_rank_table(binb, len(reads), k)
    if case == "all_on_rank0":
        n = len(reads)
        slices = read_slices(binb, world, [(0, n)] + [(n, n)] * (world - 1))
        options = {0: {"test_max_stage": 2048}}                 # rank 0 runs many chunks, the others none
    else:
        slices = read_slices(binb, world)
        options = {1: {"test_max_stage": 1024}}                 # rank 1 runs many chunks, the others one
    out = run_world(world, count_body(slices, k, options))
    check_same_table(out, want, occ)
    if case == "all_on_rank0":
        assert out[1][1] == out[2][1] == 0 and out[1][2] > 0


@pytest.mark.parametrize("k", [21, 63])
def test_offset_framing_agrees_with_fixed_stride(k):
    """a uniform stream forced through the offset-framed route (host_ragged) gives the fixed-stride route's table"""
    world = 2
    rnd = random.Random(k)
    g = "".join(rnd.choice("AGCT") for _ in range(5000))
    reads = [g[s:s + 100] for s in (rnd.randrange(0, 4900) for _ in range(3000))]
    binb = dna.reads_to_bin(reads)
    want, occ = one_rank_table(binb, len(reads), k)
    slices = read_slices(binb, world)
    fixed = run_world(world, count_body(slices, k))
    ragged = run_world(world, count_body(slices, k, {0: {"host_ragged": 1}, 1: {"host_ragged": 1}}))
    check_same_table(fixed, want, occ)
    check_same_table(ragged, want, occ)


@pytest.mark.parametrize("world", [2, 3])
def test_a_truncated_stream_fails_every_rank_and_changes_nothing(world):
    k = 31
    reads = ragged_reads(21, 1500)
    binb = dna.reads_to_bin(reads)
    slices = read_slices(binb, world)
    bad = world - 1

    def body(rank, c, hd):
        pm = DistDNAMap(hd, k, 1 << 10)
        pm.count_reads(*slices[rank])                            # something in every partition first
        before = pm.local.verify_checksum()
        b, n = slices[rank]
        if rank == bad:
            b = b[:-3]
        err = None
        try:
            pm.count_reads(b, n)
        except L.GkError as e:
            err = e.code
        after = pm.local.verify_checksum()
        pm.count_reads(*slices[rank])                            # the handles go on working
        res = (err, before, after, pm.local.verify_checksum())
        pm.close()
        return res

    out = run_ranks(world, body)
    for err, before, after, again in out:
        assert err == L.GK_E_FORMAT
        assert after == before and before[0] > 0
        assert again[2] == 2 * before[2]                         # (sum of counts: the same reads counted twice)


@pytest.mark.parametrize("world", [2, 3])
def test_an_exchange_failure_mid_stream_fails_every_rank(world):
    k = 21
    reads = ragged_reads(31, 2000)
    binb = dna.reads_to_bin(reads)
    want, occ = one_rank_table(binb, len(reads), k)
    slices = read_slices(binb, world)

    def body(rank, c, hd):
        c.set_option("test_max_stage", 1024)                     # many chunks on every rank
        if rank == 1:
            c.set_option("test_dist_fail_exchange", 4)
        pm = DistDNAMap(hd, k, 1 << 10)
        err = None
        try:
            pm.count_reads(*slices[rank])
        except L.GkError as e:
            err = (e.code, str(e))
        pm.local.clear()
        sent, owned = pm.count_reads(*slices[rank])              # the same handles, a clean count
        res = (pm.local.sorted_items(), sent, owned, count_foreign(pm.local, world, rank), err)
        pm.close()
        return res

    out = run_ranks(world, body)
    for o in out:
        assert o[4] is not None and o[4][0] < 0, o[4]
    assert "injected" in out[1][4][1]
    check_same_table(out, want, occ)


# ---- the pipeline ------------------------------------------------------------------------------------------------------

def ragged_pairs(seed, k, npairs=4000):
    """make_pairs' mates (insert 80..100), each cut at a random position: a few below k, none empty"""
    reads = make_pairs(seed, k, L=60, npairs=npairs)
    rnd = random.Random(seed + 1)
    return [r[:rnd.randint(k - 5, 60) if rnd.random() < 0.05 else rnd.randint(max(k, 30), 60)] for r in reads]


def one_rank_pipeline(binb, npairs, k, rounds, take, walk):
    c = Context(0)
    m = HipDNAMap(c, k)
    n = min(take, npairs)
    off = dna.bin_pair_offsets(binb, n)
    head = binb[:int(off[n])]
    m.count_reads(head, 2 * n)
    m.deleteAll_lt(rounds)
    good = m.size()
    g = buildGraph(k, m)
    nodes, edges, total = g.counts()
    h1, h2 = g.componentHistograms()
    kept, comps = g.retainLargest()
    g.removeBubbles(); g.simplifyGraph()
    vm = g.getGraphMap()
    sup = Support(c)
    g.walkPairs(vm, sup, head, n, walk[1], walk[2])
    sp, bad, walked = sup.sizes()
    rm, nn = g.splitBySupport(sup, walk[0])
    g.simplifyGraph()
    n2, e2, l2 = g.counts()
    stats = {"k": k, "rounds": rounds, "good_kmers": good, "graph_nodes": nodes, "graph_edges": edges, "total_edges_length": total,
             "components": comps, "max_component_size": kept, "retained_nodes": n2, "retained_edges": e2, "retained_edges_length": l2,
             "walk_pairs": {"supported_edge_pairs": sp, "bad_pairs": bad, "orientations_walked": walked, "removed_edges": rm, "new_nodes": nn},
             "components_histogram": [list(x) for x in h1], "components_histogram_2": [list(x) for x in h2]}
    res = stats, gpu_canonical(g), g.checksum()
    sup.close(); vm.close(); g.close(); m.close(); c.close()
    return res


@pytest.mark.parametrize("world,k", [(1, 21), (2, 31), (3, 21)])
def test_pipeline_over_ranks_is_the_one_rank_flow(world, k):
    reads = ragged_pairs(world + k, k)
    binb = dna.reads_to_bin(reads)
    npairs, take, rounds, walk = len(reads) // 2, len(reads) // 2 - 37, 2, (3, 60, 95)
    data = PairedEndData(npairs, binb)
    want, want_canon, want_sum = one_rank_pipeline(binb, npairs, k, rounds, take, walk)
    assert want["walk_pairs"]["orientations_walked"] > 0 and want["walk_pairs"]["supported_edge_pairs"] > 0

    def body(rank, c, hd):
        g, stats = build_graph(hd, data, k, rounds=rounds, take_first=take, retain=True, simplify=True, walk_pairs=walk)
        res = stats, gpu_canonical(g), g.checksum()
        g.close()
        return res

    out = run_world(world, body)
    n = min(take, npairs)
    off = dna.bin_pair_offsets(binb, n)
    _, occ = one_rank_table(binb[:int(off[n])], 2 * n, k)
    assert sum(o[0]["occurrences_sent"] for o in out) == occ == sum(o[0]["occurrences_owned"] for o in out)
    for stats, canon, csum in out:
        assert stats["world"] == world
        assert {x: v for x, v in stats.items() if x not in ("occurrences_sent", "occurrences_owned", "world")} == want
        assert canon == want_canon and csum == want_sum


def json_line(stdout):
    """the JSON object graph_builder prints (RCCL may print a banner line of its own to stdout first)"""
    lines = [x for x in stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, stdout
    return json.loads(lines[0])


def test_graph_builder_world_one_matches_the_plain_run(tmp_path):
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "genome_amd", "csrc"), "host"])
    k = 21
    reads = ragged_pairs(7, k)
    binf = tmp_path / "reads.bin"
    binf.write_bytes(dna.reads_to_bin(reads))
    args = [EXE, str(binf), str(len(reads) // 2), str(k), "--rounds", "2", "--take-first", str(len(reads) // 2 - 11), "--simplify",
            "--walk-pairs", "3", "60", "95"]
    plain = subprocess.run(args + ["--out", str(tmp_path / "a")], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stderr
    dist = subprocess.run(args + ["--out", str(tmp_path / "b"), "--world", "1", "--rank", "0", "--id-file", str(tmp_path / "id")],
                          capture_output=True, text=True, timeout=300)
    assert dist.returncode == 0, dist.stderr
    a, b = json_line(plain.stdout), json_line(dist.stdout)
    assert b["world"] == 1 and b["occurrences_sent"] == b["occurrences_owned"] > 0
    assert set(a) < set(b) and all(a[x] == b[x] for x in a), (a, b)
    assert a["walk_pairs"]["orientations_walked"] > 0
    for ext in (".nodes.txt", ".edges.txt"):
        assert sorted(open(str(tmp_path / "a") + ext).read().splitlines()) == sorted(open(str(tmp_path / "b") + ext).read().splitlines())
    assert len((tmp_path / "id").read_bytes()) == 128
