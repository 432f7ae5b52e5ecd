"""gk_graph_pair_distances, gk_dist_pair_distances and the `auto` range on the device (-m gpu).  `hist` and all nine classes must
equal, exactly, what tests/insert_ref.py (strings only; held to hand-computed answers by tests/test_insert_cpu.py) gives on the
ORACLE's graph of the same reads.  Fixtures: pairs_ref.make_pairs, a 2400-base genome with three planted repeats, mates of k + 9
bases, a few hundred pairs with inserts 80..100.  Every case first asserts, on the restatement alone, that the classes it is
about are populated."""
import random
import threading

import numpy as np
import pytest

from genome_amd import _lib as L
from genome_amd import dna
from genome_amd.dist import HipDist, unique_id
from genome_amd.dist_pipeline import simplify_graph
from genome_amd.dnamap import Context, HipDNAMap, HipValueMap, pos_edge
from genome_amd.freqfilter import PairedEndData
from genome_amd.graph import PAIR_CLASSES, buildGraph, insertRange
from insert_cases import E2E, E2E_MAX_INSERT, E2E_SEED, PLANTED_SEEDS, oracle_index, restate, small_pairs
from insert_ref import CLASSES, classify, insert_range, pair_distances
from oracle import pyref as R
from pairs_ref import make_pairs

pytestmark = pytest.mark.gpu
WINDOW = 4096                      # the LDS window of k_pair_distances (gk_insert.hip: PD_LDS_BINS)


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
    return m, g, g.getGraphMap()


def same(got, want):
    hist, cls = got
    assert PAIR_CLASSES == CLASSES and hist.dtype == np.uint64
    assert cls == want[1], (cls, want[1])
    assert cls["orientations"] == sum(cls[c] for c in CLASSES[1:])
    assert hist.tolist() == want[0]
    assert int(hist.sum()) == cls["counted"]


# ---- key widths --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("err", [0.0, 0.01])
@pytest.mark.parametrize("k", [21, 31, 34, 47, 64])
def test_every_key_width(ctx, k, err):
    """One word (21, 31), four bits of the high word (34), two words (47), the tagged table (64).  Error-free: every k-mer is
    kept.  1 % substitutions with the count filter at 2: the k-mers of the errors are gone from the graph, which is what
    populates unplaced and apart."""
    reads = small_pairs(100 + k, k, err=err, npairs=800 if err else 400)      # (the filter at 2 needs the coverage)
    min_count = 2 if err else 1
    npairs = len(reads) // 2
    want = restate(k, reads, reads, npairs, 128, min_count)
    assert want[1]["counted"] > 50 and want[1]["apart"] > 0 and want[1]["near_end"] > 0
    if err:
        assert want[1]["unplaced"] > 50
    m, g, vm = device_graph(ctx, k, reads, min_count)
    before = g.idFingerprint(), vm.size()
    same(g.pairDistances(vm, (dna.reads_to_bin(reads), npairs), bins=128), want)
    same(g.pairDistances(vm, PairedEndData(npairs, dna.reads_to_bin(reads)), bins=128, take_first=npairs // 3), restate(k, reads, reads, npairs // 3, 128, min_count))
    assert (g.idFingerprint(), vm.size()) == before
    vm.close(); g.close(); m.close()


# ---- stream shapes, bins, errors ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def k31(ctx):
    k = 31
    reads = small_pairs(131, k)
    index, lens = oracle_index(k, reads)
    m, g, vm = device_graph(ctx, k, reads)
    yield k, reads, index, lens, g, vm
    vm.close(); g.close(); m.close()


def test_stream_shapes(ctx, k31):
    """The fixed-stride stream is cut on the device (k_pair_keys), the ragged one on the host: the same pairs give the same
    output.  Mates shorter than k drop their pair; npairs below the stream takes a prefix; a stream that ends inside a pair is
    GK_E_FORMAT in either cut."""
    k, reads, index, lens, g, vm = k31
    npairs = len(reads) // 2
    assert {len(r) for r in reads} == {k + 9}
    want = pair_distances(k, index, lens, reads, npairs, 128)
    fixed = g.pairDistances(vm, (dna.reads_to_bin(reads), npairs), bins=128)
    same(fixed, want)
    ragged = [r[:len(r) - (i % 4) * 3] if i % 3 else r for i, r in enumerate(reads)]          # k + 9, k + 6, k + 3, k bases: the first k-mers stay
    assert {len(r) for r in ragged} == {k, k + 3, k + 6, k + 9}
    got = g.pairDistances(vm, (dna.reads_to_bin(ragged), npairs), bins=128)
    same(got, want)
    assert np.array_equal(got[0], fixed[0]) and got[1] == fixed[1]
    short = list(ragged)
    for i in (0, 7, 200, len(short) - 1):
        short[i] = short[i][:k - 1]
    short[51] = ""
    want_short = pair_distances(k, index, lens, short, npairs, 128)
    assert want_short[1]["orientations"] == 2 * (npairs - 5)
    same(g.pairDistances(vm, (dna.reads_to_bin(short), npairs), bins=128), want_short)
    for stream in (reads, ragged):
        same(g.pairDistances(vm, (dna.reads_to_bin(stream), 100), bins=128), pair_distances(k, index, lens, stream, 100, 128))
        cut = dna.reads_to_bin(stream[:201])                   # 100 pairs and one record
        with pytest.raises(L.GkError) as e:
            g.pairDistances(vm, (cut, 101), bins=128)
        assert e.value.code == L.GK_E_FORMAT
        same(g.pairDistances(vm, (cut, 100), bins=128), pair_distances(k, index, lens, stream, 100, 128))
    empty = g.pairDistances(vm, (b"", 0), bins=128)
    assert not empty[0].any() and not any(empty[1].values())


@pytest.mark.parametrize("bins", [102, 91, 2, 32, 65536])
def test_bins_decide_beyond_and_near_end(ctx, k31, bins):
    """max_dist = 101, just above the largest insert (100): near_end fills and nothing is beyond.  max_dist = 90: beyond fills.
    bins = 2 and k + 1: everything placed on one edge is beyond (D >= k > max_dist).  65536: no edge of a 2400-base genome is long
    enough, every observation is near_end."""
    k, reads, index, lens, g, vm = k31
    npairs = len(reads) // 2
    want = pair_distances(k, index, lens, reads, npairs, bins)
    c = want[1]
    if bins == 102:
        assert c["near_end"] > 20 and c["beyond"] == 0 and c["counted"] > 50
    elif bins == 91:
        assert c["beyond"] > 50 and c["counted"] > 50
    elif bins in (2, 32):
        assert c["beyond"] > 50 and c["counted"] == c["near_end"] == 0
    else:
        assert c["near_end"] > 50 and c["counted"] == c["beyond"] == 0
    same(g.pairDistances(vm, (dna.reads_to_bin(reads), npairs), bins=bins), want)


def test_arguments(ctx, k31):
    k, reads, index, lens, g, vm = k31
    binb = dna.reads_to_bin(reads)
    for bins in (0, 1, 65537):
        with pytest.raises(L.GkError) as e:
            g.pairDistances(vm, (binb, 10), bins=bins)
        assert e.value.code == L.GK_E_INVALID
    other = HipValueMap(ctx, 21, 64)
    with pytest.raises(L.GkError) as e:
        g.pairDistances(other, (binb, 10))
    assert e.value.code == L.GK_E_KLEN
    other.close()
    c2 = Context(0)
    foreign = HipValueMap(c2, k, 64)
    with pytest.raises(L.GkError) as e:
        g.pairDistances(foreign, (binb, 10))
    assert e.value.code == L.GK_E_INVALID
    foreign.close(); c2.close()


def test_reversed(ctx, k31):
    """The mates swapped and reverse-complemented: mate 1's k-mer now lies AFTER mate 2's on the edge, D = k - (insert - k) < k."""
    k, reads, index, lens, g, vm = k31
    swapped = []
    for i in range(0, len(reads), 2):
        swapped += [R.rev_comp(reads[i + 1][:k]), R.rev_comp(reads[i][:k])]
    npairs = len(swapped) // 2
    want = pair_distances(k, index, lens, swapped, npairs, 128)
    assert want[1]["reversed"] > 300 and want[1]["counted"] == 0
    same(g.pairDistances(vm, (dna.reads_to_bin(swapped), npairs), bins=128), want)


# ---- beyond the LDS window ---------------------------------------------------------------------------------------------------------

def test_distances_past_the_lds_window(ctx):
    """A 40 kbp error-free genome from tiling reads (one long unitig per strand), 300 pairs of mates with inserts 4200..4400,
    beyond the 4096 bins a workgroup keeps in LDS.  bins = 65536: exact against the restatement — where every observation is
    near_end, no edge of this genome being 65535 - k bases long.  bins = 4500 on the same pairs: the distances are counted, all of
    them in bins the kernel reaches by global atomics only."""
    k, G, Lr = 31, 40000, 100
    rnd = random.Random(4096)
    genome = "".join(rnd.choice("AGCT") for _ in range(G))
    tiles = []
    for s in list(range(0, G - Lr + 1, 25)) + [G - Lr]:
        tiles += [genome[s:s + Lr], R.rev_comp(genome[s:s + Lr])]
    mates = []
    for _ in range(300):
        ins = rnd.randint(4200, 4400)
        s = rnd.randrange(0, G - ins)
        frag = genome[s:s + ins]
        if rnd.random() < 0.5:
            frag = R.rev_comp(frag)
        mates += [frag[:k + 9], R.rev_comp(frag)[:k + 9]]
    index, lens = oracle_index(k, tiles)
    assert max(lens) > 30000
    m, g, vm = device_graph(ctx, k, tiles)
    pbin = dna.reads_to_bin(mates)
    want = pair_distances(k, index, lens, mates, 300, 65536)
    assert want[1]["near_end"] == 600 and want[1]["counted"] == 0
    same(g.pairDistances(vm, (pbin, 300), bins=65536), want)
    want = pair_distances(k, index, lens, mates, 300, 4500)
    assert want[1]["counted"] > 400 and sum(want[0][:WINDOW]) == 0 and want[1]["near_end"] > 0
    got = g.pairDistances(vm, (pbin, 300), bins=4500)
    same(got, want)
    assert insertRange(got[0], trim=0, min_observations=1)[:2] == insert_range(want[0], 0, 1)[:2]
    assert 4200 <= insertRange(got[0], trim=0, min_observations=1)[0] and insertRange(got[0], trim=0, min_observations=1)[1] <= 4400
    # both sides of the window's edge in one call: inserts 4090..4100
    edge = []
    for ins in range(4090, 4101):
        for s in (1000, 7000, 20000):
            frag = genome[s:s + ins]
            edge += [frag[:k], R.rev_comp(frag)[:k]]
    want = pair_distances(k, index, lens, edge, len(edge) // 2, 4200)
    assert want[0][4090:4101] == [6] * 11
    same(g.pairDistances(vm, (dna.reads_to_bin(edge), len(edge) // 2), bins=4200), want)
    vm.close(); g.close(); m.close()


# ---- repetitive, ambiguous, dead edges: a hand-filled position map ---------------------------------------------------------------

def test_hand_filled_position_map(ctx):
    """A fresh graph holds a k-mer once: lists of more than one position come from a position map filled by hand with positions
    that are valid in the graph.  16 entries are looked at and 17 are not; two combinations on one edge are ambiguous; a position
    on an edge that has been removed is GK_E_STATE."""
    k = 21
    reads = small_pairs(121, k)
    m, g, _vm = device_graph(ctx, k, reads)
    _vm.close()
    ids = np.arange(g.idBounds()[1], dtype=np.uint32)
    info = g.edgesById(ids)
    lens = [int(x) for x in info["len"]]
    long_edges = [int(e) for e in ids if info["alive"][e] and lens[e] >= 60]
    assert len(long_edges) >= 2
    E, F = long_edges[:2]
    rnd = random.Random(5)
    names = "X16 X17 A2 Y ONE Z".split()
    key = {n: "".join(rnd.choice("AGCT") for _ in range(k)) for n in names}
    assert len({key[n] for n in names} | {R.rev_comp(key[n]) for n in names}) == 2 * len(names)
    lists = {"X16": [("E", F, d) for d in range(1, 17)], "X17": [("E", F, d) for d in range(1, 18)], "A2": [("E", E, 3), ("E", E, 7)],
             "Y": [("E", E, 20)], "ONE": [("E", E, 3)], "Z": [("E", F, 30)]}
    vm = HipValueMap(ctx, k, 256)
    for n in names:
        vm.putNew_batch([key[n]] * len(lists[n]), [pos_edge(e, d) for _, e, d in lists[n]])
    assert vm.size() == 16 + 17 + 2 + 1 + 1 + 1
    bins = k + 30                                              # max_dist = k + 29: dist(a) = 3 is near the end of edges below 33 bases only
    cases = [("X16", "Y", "apart"), ("X17", "Y", "repetitive"), ("Y", "X17", "repetitive"), ("X16", "Z", "ambiguous"), ("A2", "Y", "ambiguous"),
             ("ONE", "Y", "counted"), ("Y", "ONE", "reversed"), ("ONE", "Z", "apart"), ("X17", "X17", "repetitive")]
    stream, want_hist, want = [], [0] * bins, dict.fromkeys(CLASSES, 0)
    for a, b, name in cases:
        stream += [key[a], R.rev_comp(key[b])]
        c, D = classify(lists[a], lists[b], k, lens, bins - 1)
        assert c == name
        want[c] += 1
        want["unplaced"] += 1                                  # orientation 1 looks up the reverse complements: not in the map
        want["orientations"] += 2
        if c == "counted":
            want_hist[D] += 1
    assert want_hist[17 + k] == 1
    same(g.pairDistances(vm, (dna.reads_to_bin(stream), len(cases)), bins=bins), (want_hist, want))
    assert g.removeEdgesById([F]) == 1
    with pytest.raises(L.GkError) as e:
        g.pairDistances(vm, (dna.reads_to_bin(stream), len(cases)), bins=bins)
    assert e.value.code == L.GK_E_STATE
    same(g.pairDistances(vm, (dna.reads_to_bin(stream[10:14]), 2), bins=bins), ([0] * (17 + k) + [1] + [0] * (bins - 18 - k),
                                                                                 dict(want, orientations=4, unplaced=2, counted=1, reversed=1, apart=0, repetitive=0, ambiguous=0)))
    vm.close(); g.close(); m.close()


# ---- the grid cap -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", [1, 3])
def test_grid_cap(k31, cap):
    """800 orientations on 1 and on 3 workgroups of 256 lanes: every lane takes several trips, the last one partly past the end."""
    k, reads, index, lens, g, vm = k31
    npairs = len(reads) // 2
    assert 2 * npairs > 3 * 256
    ctx = g.ctx
    want = pair_distances(k, index, lens, reads, npairs, 102)
    free = g.pairDistances(vm, (dna.reads_to_bin(reads), npairs), bins=102)
    ctx.set_option("test_max_grid", cap)
    try:
        uses = ctx.grid_cap_uses()
        capped = g.pairDistances(vm, (dna.reads_to_bin(reads), npairs), bins=102)
        assert ctx.grid_cap_uses() > uses
    finally:
        ctx.set_option("test_max_grid", 0)
    same(capped, want)
    assert np.array_equal(capped[0], free[0]) and capped[1] == free[1]


# ---- planted truth -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", sorted(PLANTED_SEEDS))
def test_planted_inserts_are_found(ctx, k):
    reads = small_pairs(PLANTED_SEEDS[k], k)
    npairs = len(reads) // 2
    want = restate(k, reads, reads, npairs, 128)
    lo, hi, _ = insert_range(want[0], 0, 1)
    assert 80 <= lo and hi <= 100 and want[1]["counted"] > 100          # the seed's promise, on the restatement alone
    m, g, vm = device_graph(ctx, k, reads)
    hist, cls = g.pairDistances(vm, (dna.reads_to_bin(reads), npairs), bins=128)
    same((hist, cls), want)
    lo, hi, med = insertRange(hist, trim=0, min_observations=1)
    assert 80 <= lo and hi <= 100 and lo <= med <= hi
    assert insertRange(hist) is None                                     # fewer than the default 1000 observations: no estimate
    vm.close(); g.close(); m.close()


# ---- end to end ----------------------------------------------------------------------------------------------------------------------

def e2e_pairs(ins):
    return make_pairs(E2E_SEED, E2E["k"], glen=E2E["glen"], nrep=E2E["nrep"], L=E2E["L"], npairs=E2E["npairs"], ins=ins)


def test_simplify_graph_with_an_estimated_range(ctx, tmp_path):
    """inserts 180..250: the trim-0 estimate is exactly the reference's range, and the auto run IS the 180..250 run.  inserts
    300..340: the reference's range supports nothing (every walked orientation is bad), the estimated one does."""
    k = E2E["k"]
    hd = HipDist(ctx, 0, 1, unique_id())
    reads = e2e_pairs((180, 250))
    want = restate(k, reads, reads, len(reads) // 2, E2E_MAX_INSERT + 1)
    assert insert_range(want[0], 0, 1)[:2] == (180, 250)
    data = PairedEndData(len(reads) // 2, dna.reads_to_bin(reads))
    m, g, vm = device_graph(ctx, k, reads)
    path = tmp_path / "a.graph"
    g.save(path)
    vm.close(); g.close(); m.close()
    ga, sa = simplify_graph(hd, path, data, 3, lo="auto", max_insert=E2E_MAX_INSERT, trim=0, min_observations=1)
    gn, sn = simplify_graph(hd, path, data, 3, 180, 250)
    est = sa["walk_pairs"].pop("insert_range")
    assert (est["lo"], est["hi"], est["estimated"]) == (180, 250, True) and est["classes"] == want[1]
    assert "insert_range" not in sn["walk_pairs"] and sa == sn
    assert ga.checksum() == gn.checksum() and ga.counts() == gn.counts()
    ga.close(); gn.close()
    # no estimate: the fallback is the reference's range, and says so
    gf, sf = simplify_graph(hd, path, data, 3, lo="auto", max_insert=E2E_MAX_INSERT, min_observations=10 ** 6)
    est = sf["walk_pairs"].pop("insert_range")
    assert (est["lo"], est["hi"], est["median"], est["estimated"]) == (180, 250, None, False) and sf == sn
    gf.close()
    # another library
    reads = e2e_pairs((300, 340))
    data = PairedEndData(len(reads) // 2, dna.reads_to_bin(reads))
    m, g, vm = device_graph(ctx, k, reads)
    path = tmp_path / "b.graph"
    g.save(path)
    vm.close(); g.close(); m.close()
    ga, sa = simplify_graph(hd, path, data, 3, lo="auto", max_insert=400, min_observations=1000)
    gn, sn = simplify_graph(hd, path, data, 3)
    est = sa["walk_pairs"]["insert_range"]
    assert est["estimated"] and 300 <= est["lo"] <= est["median"] <= est["hi"] <= 340
    assert sn["walk_pairs"]["bad_pairs"] > 0 and sa["walk_pairs"]["bad_pairs"] < sn["walk_pairs"]["bad_pairs"]
    assert sa["walk_pairs"]["supported_edge_pairs"] > sn["walk_pairs"]["supported_edge_pairs"]
    ga.close(); gn.close(); hd.close()


# ---- ranks ---------------------------------------------------------------------------------------------------------------------------

def _run_ranks(world, body, timeout=120):
    """`body(rank, ctx, hd)` on one thread per rank over the loopback transport (as tests/test_spectrum_gpu.py does)"""
    id128 = bytes(random.Random(world * 7919 + 3).getrandbits(8) for _ in range(128))
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

    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=timeout)
    assert not any(t.is_alive() for t in threads), "a rank is stuck"
    assert not errors, errors
    return out


@pytest.mark.parametrize("world,k", [(2, 31), (3, 47)])
def test_ranks_over_the_loopback_transport(ctx, world, k):
    """Every rank's gk_dist_pair_distances over its share is the one-rank call over all pairs.  Then one rank passes no position
    map (a real local failure: GK_E_INVALID there): it still enters the collective, EVERY rank gets an error, nobody hangs, and
    the handle works afterwards."""
    reads = small_pairs(700 + k, k, err=0.01, npairs=800)
    npairs = len(reads) // 2
    want = restate(k, reads, reads, npairs, 128, 2)
    assert want[1]["counted"] > 50 and want[1]["unplaced"] > 0
    m, g, vm = device_graph(ctx, k, reads, 2)
    one = g.pairDistances(vm, (dna.reads_to_bin(reads), npairs), bins=128)
    same(one, want)
    vm.close(); g.close(); m.close()
    bad = world - 1

    def body(rank, c, hd):
        m_, g_, vm_ = device_graph(c, k, reads, 2)
        a, b = npairs * rank // world, npairs * (rank + 1) // world
        share = dna.reads_to_bin(reads[2 * a:2 * b])
        first = hd.pair_distances(g_, vm_, share, b - a, bins=128)
        err = None
        try:
            hd.pair_distances(g_, None if rank == bad else vm_, share, b - a, bins=128)
        except L.GkError as e:
            err = e.code
        again = hd.pair_distances(g_, vm_, share, b - a, bins=102)
        vm_.close(); g_.close(); m_.close()
        return first, err, again

    want102 = restate(k, reads, reads, npairs, 102, 2)
    for rank, (first, err, again) in enumerate(_run_ranks(world, body)):
        same(first, want)
        assert np.array_equal(first[0], one[0]) and first[1] == one[1]
        assert err == (L.GK_E_INVALID if rank == bad else L.GK_E_COMM), (rank, err)
        same(again, want102)
