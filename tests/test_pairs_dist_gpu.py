"""The paired-end stage over N ranks (-m gpu): adding up and merging supports on one device (gk_support_add / _merge), and the
collective that sums every rank's support into every rank's (gk_dist_reduce_support).

The support is a sum over read pairs and every pair orientation is walked on one rank only, so the element-wise sum of the
ranks' supports IS the support of one rank walking all the pairs: bit-exact against the single-rank gk_graph_walk_pairs (itself
checked against the oracle in test_pairs_gpu.py), and by content against the oracle.

The replicas need not number their nodes and edges alike, and in general do not: gk_graph_build numbers the terminal k-mers in
the slot order of the table it is given (and the slot a key lands in depends on the order of racing CAS inserts), and reserves
its output ranges with atomic cursors once a graph spans several workgroups.  The reduce therefore moves the pairs in a
canonical numbering — live edges ordered by (start k-mer, first base) — and checks that the replicas hold the same EDGES (a
content fingerprint), not the same ids.  Here the odd ranks build their replica on purpose from a table of another layout (all
reads counted on the rank's own context, another capacity).  Bit-exact by id, each rank's summed support is therefore compared
with one walk of ALL pairs on that rank's own replica; the counters and the content are compared with the single-device run and
the oracle, and the graph after split + simplify with the oracle's.

World > 1 runs over the test library's loopback transport (ranks as threads of this process on one device); world 1 over
RCCL, the product transport."""
import random
import threading
from collections import Counter

import numpy as np
import pytest

from genome_amd import _lib as L
from genome_amd import dna
from genome_amd.dist import DistDNAMap, HipDist, unique_id
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.graph import Support, buildGraph
from oracle import oracle as O
from test_pairs_gpu import gpu_canonical, gpu_support_by_content, make_pairs, oracle_canonical, oracle_support_by_content

pytestmark = pytest.mark.gpu

READ_LEN = 40                                      # make_pairs' mates: fixed-length `.bin` records of 1 + 10 bytes
U32_MAX = (1 << 32) - 1


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def triples(sup):
    """the support by id: (e1, e2, count) sorted, as one array"""
    e1, e2, cnt = sup.items()
    o = np.lexsort((e2, e1))
    return np.stack([e1[o], e2[o], cnt[o]]).astype(np.uint64)


def snapshot(sup):
    return triples(sup), sup.sizes()


def same(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1]


def as_counter(t):
    return Counter({(int(a), int(b)): int(c) for a, b, c in zip(*t)})


def run_ranks(world, body, timeout=300):
    """`body(rank, ctx, hd)` on one thread per rank over the loopback transport -> the ranks' results; fails on a stuck rank.
    The bodies return data and the checks run here, so that a failed check cannot leave the other ranks in a collective."""
    id128 = bytes(random.Random(world * 104729 + 7).getrandbits(8) for _ in range(128))
    out, errors = [None] * world, []

    def run(rank):
        try:
            c = Context(0)
            hd = HipDist(c, rank, world, id128, loopback=True)
            out[rank] = body(rank, c, hd)
            hd.barrier()
            hd.close(); c.close()
        except BaseException as e:          # noqa: BLE001 — reported by the main thread
            errors.append((rank, repr(e)))

    threads = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=timeout)
    assert not any(t.is_alive() for t in threads), "a rank is stuck"
    assert not errors, errors
    return out


def pair_shares(npairs, world):
    """contiguous, uneven shares of the pairs; rank world // 2 gets none"""
    w = [0 if r == world // 2 else r + 1 for r in range(world)]
    cuts = [0]
    for r in range(world):
        cuts.append(npairs if r == world - 1 else cuts[-1] + npairs * w[r] // sum(w))
    return [(cuts[r], cuts[r + 1]) for r in range(world)]


def read_shares(nreads, world):
    return [(nreads * r // world, nreads * (r + 1) // world) for r in range(world)]


def rank_graph(c, hd, k, binb, nreads, rank, world, classified, retain, other_layout=False, read_len=READ_LEN):
    """this rank's reads counted through the partitioned map, filtered, gathered, built (and its largest component kept).
    other_layout: the gather still runs (it is collective), but the replica is built from all reads counted on this rank's own
    context in a table of another capacity — another slot layout, hence (in general) other ids."""
    a, b = read_shares(nreads, world)[rank]
    stride = 1 + (read_len + 3) // 4
    rec = np.frombuffer(binb, np.uint8)[a * stride:b * stride]
    d = c.alloc(max(rec.size, 1) + 64)
    if rec.size:
        c.upload(d, np.ascontiguousarray(rec))
    pm = DistDNAMap(hd, k, 1 << 10)
    pm.count_reads_dev(d, b - a, read_len)
    pm.deleteAll_lt(2)
    full = pm.gathered(classified=classified)
    if other_layout:
        full.close()
        full = HipDNAMap(c, k, (1 << 15) * (rank + 1))
        full.count_reads(binb, nreads)
        full.deleteAll_lt(2)
    g = buildGraph(k, full)
    if retain:
        g.retainLargest()
    pm.close(); c.free(d)
    return full, g


def walk_share(c, g, vm, binb, share, rng):
    sup = Support(c)
    a, b = share
    if b > a:
        g.walkPairs(vm, sup, dna.bin_pairs(binb, a, b), b - a, *rng)
    return sup


# ---- one device ---------------------------------------------------------------------------------------------------------

def one_device_setup(ctx, k=21, seed=1, rng=(60, 95)):
    reads = make_pairs(seed, k)
    binb = dna.reads_to_bin(reads)
    m = HipDNAMap(ctx, k)
    m.count_reads(binb, len(reads))
    m.deleteAll_lt(2)
    g = buildGraph(k, m)
    return m, g, g.getGraphMap(), binb, len(reads) // 2, rng


def test_add_reproduces_an_exported_support(ctx):
    m, g, vm, binb, npairs, rng = one_device_setup(ctx)
    sup = Support(ctx)
    g.walkPairs(vm, sup, binb, npairs, *rng)
    want = snapshot(sup)
    assert want[1][0] > 0 and want[1][2] > 0
    e1, e2, cnt = sup.items()
    s2 = Support(ctx)
    s2.add(e1, e2, cnt, want[1][1], want[1][2])
    assert same(snapshot(s2), want)
    # duplicates in one list add up, and so do two calls
    s3 = Support(ctx)
    s3.add(np.concatenate([e1, e1]), np.concatenate([e2, e2]), np.concatenate([cnt, cnt]), 1, 2)
    s3.add(e1, e2, cnt)
    t = triples(s3)
    assert np.array_equal(t[:2], want[0][:2]) and np.array_equal(t[2], 3 * want[0][2])
    assert s3.sizes() == (want[1][0], 1, 2)
    # the host copy the split reads is refreshed after an add
    s2.add([], [], [], 5, 0)
    assert s2.sizes()[1] == want[1][1] + 5 and np.array_equal(triples(s2), want[0])
    for s in (sup, s2, s3):
        s.close()
    vm.close(); g.close(); m.close()


def test_merge_of_two_halves_is_the_whole(ctx):
    m, g, vm, binb, npairs, rng = one_device_setup(ctx, k=31, seed=3, rng=(50, 85))
    whole = Support(ctx)
    g.walkPairs(vm, whole, binb, npairs, *rng)
    half = npairs // 3
    a, b = walk_share(ctx, g, vm, binb, (0, half), rng), walk_share(ctx, g, vm, binb, (half, npairs), rng)
    b_before = snapshot(b)
    a.merge(b)
    assert same(snapshot(a), snapshot(whole))
    assert same(snapshot(b), b_before)                        # src is unchanged
    # merging into an empty support copies; an empty src changes nothing
    e = Support(ctx)
    e.merge(whole)
    assert same(snapshot(e), snapshot(whole))
    e.merge(Support(ctx))
    assert same(snapshot(e), snapshot(whole))
    # the split on the merged support is the split on the whole one
    assert g.splitBySupport(a, 3) == g.splitBySupport(whole, 3)
    with pytest.raises(L.GkError) as err:
        a.merge(a)
    assert err.value.code == L.GK_E_INVALID
    for s in (whole, a, b, e):
        s.close()
    vm.close(); g.close(); m.close()


def test_a_count_that_would_pass_u32_is_refused_and_nothing_changes(ctx):
    dst = Support(ctx)
    dst.add([1, 5], [2, 6], [U32_MAX - 10, 7], 3, 4)
    before = snapshot(dst)
    src = Support(ctx)
    src.add([1, 3], [2, 4], [11, 9])
    with pytest.raises(L.GkError) as err:
        dst.merge(src)
    assert err.value.code == L.GK_E_CAPACITY
    assert same(snapshot(dst), before)
    with pytest.raises(L.GkError) as err:
        dst.add([9, 1], [9, 2], [1, 11])                     # the list's own pair is fine, (1, 2) would wrap
    assert err.value.code == L.GK_E_CAPACITY
    assert same(snapshot(dst), before)
    with pytest.raises(L.GkError) as err:
        dst.add([8, 8], [8, 8], [U32_MAX, 1])                 # duplicates in the list that wrap among themselves
    assert err.value.code == L.GK_E_CAPACITY
    assert same(snapshot(dst), before)
    dst.add([1], [2], [10])                                   # exactly 2^32-1 is a count
    t = as_counter(triples(dst))
    assert t[(1, 2)] == U32_MAX and t[(5, 6)] == 7 and dst.sizes() == (2, 3, 4)
    src.close(); dst.close()


def test_id_fingerprint_sees_ids_and_liveness(ctx):
    m, g, vm, binb, npairs, rng = one_device_setup(ctx)
    fp = g.idFingerprint()
    assert fp == g.idFingerprint()
    ne = g.counts()[1]
    live = np.flatnonzero(g.edgesById(np.arange(g.idBounds()[1]))["alive"])
    assert g.removeEdgesById([int(live[len(live) // 2])]) == 1 and g.counts()[1] == ne - 1
    assert g.idFingerprint() != fp
    vm.close(); g.close(); m.close()


# ---- N ranks ----------------------------------------------------------------------------------------------------------

# make_pairs' knobs of the rows at the reference's range: 150-base mates with 0.5 % errors over an 8 kbp genome, inserts whose walk
# distance (insert - k) lies inside 180..250 (test_pairs_shapes_gpu.py's fixture); the other rows keep make_pairs' defaults
def wide_fixture(k, rng):
    return dict(glen=8000, nrep=4, L=150, npairs=6000, err=0.005, ins=(k + 185, k + 245)) if rng == (180, 250) else {}


@pytest.mark.parametrize("world,k,seed,rng,classified", [(2, 21, 1, (60, 95), True), (3, 31, 3, (50, 85), False), (8, 35, 4, (50, 80), True),
                                                         (2, 55, 5, (180, 250), True), (3, 64, 6, (180, 250), False)])
def test_reduce_over_ranks_equals_one_rank_and_the_oracle(world, k, seed, rng, classified):
    fx = wide_fixture(k, rng)
    reads = make_pairs(seed, k, **fx)
    read_len = fx.get("L", READ_LEN)
    assert {len(r) for r in reads} == {read_len}
    binb = dna.reads_to_bin(reads)
    nreads, npairs = len(reads), len(reads) // 2
    # one rank, all pairs
    c0 = Context(0)
    m = HipDNAMap(c0, k)
    m.count_reads(binb, nreads); m.deleteAll_lt(2)
    g1 = buildGraph(k, m)
    g1.retainLargest()
    fp1 = g1.idFingerprint()
    vm1 = g1.getGraphMap()
    sup1 = Support(c0)
    g1.walkPairs(vm1, sup1, binb, npairs, *rng)
    want = snapshot(sup1)
    # the oracle
    ref = O.PMap(k, 1)
    ref.count_reads(binb, nreads); ref.delete_lt(2)
    og = O.Graph(ref)
    og.retain_largest()
    assert gpu_canonical(g1) == oracle_canonical(og)
    osup = O.Support()
    walked = og.walk_pairs(osup, binb, npairs, *rng)
    want_content = oracle_support_by_content(og, k, osup)
    assert want[1][1:] == (osup.bad_pairs(), walked) and max(want_content.values()) >= 3
    osplit = og.split_by_support(osup, 3)                     # (the oracle's includes simplifyGraph)
    want_graph = oracle_canonical(og)
    shares = pair_shares(npairs, world)
    assert shares[world // 2][0] == shares[world // 2][1] and len({b - a for a, b in shares}) > 1

    def body(rank, c, hd):
        full, g = rank_graph(c, hd, k, binb, nreads, rank, world, classified, retain=True, other_layout=rank % 2 == 1, read_len=read_len)
        vm = g.getGraphMap()
        s_all = walk_share(c, g, vm, binb, (0, npairs), rng)   # one walk of every pair on THIS replica: the by-id reference
        one = snapshot(s_all)
        s_all.close()
        sup = walk_share(c, g, vm, binb, shares[rank], rng)
        mine = snapshot(sup)
        fp = g.idFingerprint()
        hd.reduce_support(g, sup)
        res = {"fp": fp, "fp_after": g.idFingerprint(), "mine": mine, "sum": snapshot(sup), "content": gpu_support_by_content(g, k, sup), "one": one}
        res["split"] = g.splitBySupport(sup, 3)
        g.simplifyGraph()
        res["checksum"], res["counts"], res["canon"] = g.checksum(), g.counts(), gpu_canonical(g)
        sup.close(); vm.close(); g.close(); full.close()
        return res

    out = run_ranks(world, body)
    assert sum(o["mine"][1][2] for o in out) == want[1][2]                 # every orientation was walked on exactly one rank
    assert out[world // 2]["mine"][1] == (0, 0, 0)
    for o in out:
        assert o["fp"] == o["fp_after"]                         # the reduce renumbers nothing
        assert same(o["sum"], o["one"])                         # by id: one walk of everything on this replica
        assert o["sum"][1] == want[1]                          # the counters of the single-device run
        if o["fp"] == fp1:                                     # a replica numbered like the single-device one: bit-exact against it too
            assert same(o["sum"], want)
        assert o["content"] == want_content == gpu_support_by_content(g1, k, sup1)
        assert o["split"] == osplit and osplit[1] > 0
        assert o["checksum"] == out[0]["checksum"] and o["counts"] == out[0]["counts"]
        assert o["canon"] == want_graph
    sup1.close(); vm1.close(); g1.close(); m.close(); c0.close()


@pytest.mark.parametrize("case", ["diverged_replica", "null_support", "late_failure", "overflow"])
@pytest.mark.parametrize("world", [2, 3])
def test_every_rank_fails_together_and_the_handles_recover(world, case):
    """(a) one rank's replica lost an edge: GK_E_STATE everywhere; (b) one rank passes no support; (c) one rank fails its owner
    merge after the records were exchanged (test_dist_fail_reduce); (d) two ranks' counts of one pair sum past 2^32-1:
    GK_E_CAPACITY everywhere.  Every rank raises from the same call, nobody is stuck, every support is unchanged, and the same
    handles then complete a correct reduce: the sum of what the ranks held."""
    k, rng = 21, (60, 95)
    reads = make_pairs(9, k, npairs=2000)
    binb = dna.reads_to_bin(reads)
    nreads, npairs = len(reads), len(reads) // 2
    shares = pair_shares(npairs, world)
    odd = world - 1                                            # the rank that is different

    def body(rank, c, hd):
        full, g = rank_graph(c, hd, k, binb, nreads, rank, world, False, retain=False)
        vm = g.getGraphMap()
        sup = walk_share(c, g, vm, binb, shares[rank], rng)
        mine = snapshot(sup)
        target, arg, extra = g, sup, None
        if case == "diverged_replica" and rank == odd:
            target = buildGraph(k, full)                       # a second replica that then loses one edge
            live = np.flatnonzero(target.edgesById(np.arange(target.idBounds()[1]))["alive"])
            assert target.removeEdgesById([int(live[0])]) == 1
        elif case == "null_support" and rank == odd:
            arg = None
        elif case == "late_failure" and rank == odd:
            c.set_option("test_dist_fail_reduce", 1)
        elif case == "overflow":
            extra = Support(c)
            if rank < 2:
                extra.add([3], [4], [(1 << 31) + 5])
            extra.add([rank], [rank + 1], [1])
            arg = extra
        arg_before = snapshot(arg) if arg is not None else None
        err = None
        try:
            hd.reduce_support(target, arg)
        except L.GkError as e:
            err = (e.code, str(e))
        unchanged = arg is None or same(snapshot(arg), arg_before)
        still = same(snapshot(sup), mine)
        hd.reduce_support(g, sup)                              # the same handles, a correct reduce
        res = (err, unchanged, still, mine, snapshot(sup))
        if target is not g:
            target.close()
        if extra is not None:
            extra.close()
        sup.close(); vm.close(); g.close(); full.close()
        return res

    out = run_ranks(world, body)
    total = Counter()
    for o in out:
        total.update(as_counter(o[3][0]))
    want_sizes = (len(total), sum(o[3][1][1] for o in out), sum(o[3][1][2] for o in out))
    for rank, (err, unchanged, still, _mine, after) in enumerate(out):
        assert err is not None, (case, rank)
        if case == "diverged_replica":
            assert err[0] == L.GK_E_STATE, err
        elif case == "overflow":
            assert err[0] == L.GK_E_CAPACITY, err
        elif case == "null_support":
            assert err[0] == (L.GK_E_INVALID if rank == odd else L.GK_E_COMM), err
        else:
            assert ("injected" in err[1]) == (rank == odd), err
        assert unchanged and still, (case, rank)
        assert as_counter(after[0]) == total and after[1] == want_sizes


def test_world_one_over_rccl_is_the_identity(ctx):
    m, g, vm, binb, npairs, rng = one_device_setup(ctx)
    hd = HipDist(ctx, 0, 1, unique_id())
    sup = Support(ctx)
    g.walkPairs(vm, sup, binb, npairs, *rng)
    before, fp = snapshot(sup), g.idFingerprint()
    hd.reduce_support(g, sup)
    assert same(snapshot(sup), before) and g.idFingerprint() == fp
    with pytest.raises(L.GkError) as err:
        hd.reduce_support(g, None)
    assert err.value.code == L.GK_E_INVALID
    hd.reduce_support(g, sup)
    assert same(snapshot(sup), before)
    sup.close(); hd.close(); vm.close(); g.close(); m.close()
